/*
 * ce_api.h -- C ABI of the MI355X-native frequency-aware cached EmbeddingBag.
 *
 * The reference (hpcaitech/CachedEmbedding) has no FFI: its boundary for this path is a
 * Python nn.Module API implemented by ColossalAI's CachedParamMgr / CachedEmbeddingBag in
 * pure torch ops.  Each entry point below replaces one of those torch-op sequences; the
 * Python mirror in cachedembedding_amd/ (ctypes) is what a reference maintainer binds
 * (see INTEGRATION.md).  Citations are relative to /root/reference; "[A.x]" refers to the
 * upstream semantics recorded in SURVEY.md Appendix A.
 *
 * Conventions: plain pointers and sizes only (no torch types); every device pointer is a
 * raw HIP device address; `stream` is a hipStream_t passed as void*; all work is enqueued
 * asynchronously on that stream with NO hidden host synchronisation unless a function
 * says it blocks; every function returns an int status (CE_OK == 0) and
 * ce_last_error() gives the message of the last failure on the calling thread.
 * Handles are not thread-safe (the reference is single-threaded per process too).
 */
#ifndef CE_API_H
#define CE_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CE_API_VERSION 6

/* status codes */
#define CE_OK 0
#define CE_ERR_INVALID 1     /* bad argument */
#define CE_ERR_HIP 2         /* a HIP runtime call failed */
#define CE_ERR_CAPACITY 3    /* unique rows of one prepare_ids call exceed cuda_row_num:
                                the reference's AssertionError caught at
                                benchmark/benchmark_cache.py:106-108 */
#define CE_ERR_NOMEM 4
#define CE_ERR_UNSUPPORTED 5
#define CE_ERR_RANGE 6       /* an id outside [0, num_embeddings) */

/* EvictionStrategy (recsys/models/dlrm.py:66,80) */
#define CE_EVICT_DATASET 0
#define CE_EVICT_LFU 1
/* Least recently used, at the grain of a call (an addition to API 6).
 *  - The last use of a resident row is the most recent ce_cache_prepare_ids-family call (plain, _keys, _begin /
 *    _finish, padded, captured) that named it; being admitted counts as being named.  A window call is one call:
 *    all its batches share one recency.  Only the order of calls matters.  ce_cache_lookup_slots is not a use, and a
 *    padding id (-1 on the padded entries) names nothing.
 *  - Rows placed by ce_cache_preload have never been used and are older than every used row.
 *  - The k victims of a call are the k resident, unprotected slots with the oldest last use (protection as for the
 *    other strategies: the call's own rows plus those used within protect_depth calls).  Among slots with the same
 *    last use the HIGHER slot leaves first: a preload by frequency puts the i-th most frequent row into slot i and
 *    never-used rows all tie, so the least frequent preloaded rows leave first.
 *  - A failed call (bad id, capacity) on the per-lookup front keeps the stamps it wrote, so it counts as a use of the
 *    resident rows it named; on the bitmap front a failed call stamps nothing and is no use.
 *  - freq_cnter is neither needed nor touched (NULL is accepted) and ce_cache_set_freq_bound does nothing.
 *  - The recency is the call number modulo 2^30, as protect_depth's stamp is: the order is defined for fewer than
 *    2^30 calls (prepare_ids, preload and flush together) on one handle. */
#define CE_EVICT_LRU 2

/* nn.EmbeddingBag mode (recsys/models/dlrm.py:74 passes 'sum') */
#define CE_MODE_SUM 0
#define CE_MODE_MEAN 1

/* Activation dtype of the bag kernels' output / incoming gradient (the ce_*_act entries; additions to API 6).  The
 * table, the accumulation and every update stay fp32; only what the forward stores and the backward reads changes. */
#define CE_ACT_F32 0
#define CE_ACT_BF16 1    /* bfloat16: round-to-nearest-even on the store, NaN stays NaN */
#define CE_ACT_F16 2     /* IEEE half: round-to-nearest-even, values beyond 65504 become inf */

/* how missed / evicted rows move between the host table and the HBM cache */
#define CE_TRANSPORT_ZEROCOPY 0  /* swap kernels read/write the mapped pinned host table over PCIe */
#define CE_TRANSPORT_STAGED 1    /* host threads gather/scatter through pinned staging + hipMemcpyAsync */
#define CE_TRANSPORT_WORKER 2    /* both directions leave the CUs: evictions are packed in HBM by the cache op, copied
                                    out with pinned hipMemcpyAsync (SDMA) on a private stream and scattered into the
                                    host table by a worker thread inside the library; missed rows are brought into
                                    an HBM staging block under the control of a second worker thread -- it waits for
                                    the miss list and for earlier write-backs to land, then either launches a
                                    small kernel on a private stream that reads them out of the mapped table
                                    (default; it does not wait for the write-back of the call just before: a row that
                                    call evicted is taken out of its staging block, still in HBM), or gathers them
                                    into pinned staging and copies that with
                                    hipMemcpyAsync (CE_WORKER_ADMIT=sdma, and tables without a device mapping) --
                                    and the cache-op stream waits for them in a hipStreamWaitValue64 after it has
                                    selected and staged the victims; the arrived rows are then copied into their
                                    slots, the maps updated and the call's slots (and keys) written (CE_EARLY_MAPS=1:
                                    maps, slots and keys before the wait).  An admission the worker reports lost (a
                                    HIP call of its own failed / timed out) gives the call CE_ERR_HIP with nothing
                                    marked resident; every later call fails.  prepare_ids stays
                                    one asynchronous call, but returns before the host table has the evicted rows
                                    (ce_cache_writeback_wait / ce_cache_flush make it current).  Not capture-safe.
                                    The library does not trust the environment for this: the first call on a stream
                                    self-tests that its copy streams run while that stream is parked (falls back to
                                    ZEROCOPY with a message otherwise), every wait on a worker has a deadline
                                    (CE_WORKER_TIMEOUT_S, default 30 s), and an admission that fails or times out
                                    releases the stream with the call flagged CE_ERR_HIP and nothing admitted. */

typedef void* ce_stream_t; /* hipStream_t */
typedef struct ce_cache ce_cache_t;

int ce_version(void);
/* CPUs this process may use: hardware threads capped by the affinity mask and the cgroup CPU quota (what the
 * library sizes its helper-thread pools against). */
int32_t ce_cpu_budget(void);
const char* ce_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Side stream for the cache manager (the "Stream1" lane of pics/prefetch.png).  The cache op is
 * PCIe/latency bound, the training kernels HBM bound; if both share all 256 CUs the cache op's
 * resident waves take wave slots from training.  ce_stream_create_cu_mask returns a HIP stream
 * restricted to the CUs whose bits are set in cu_mask (word w bit b = CU 32*w + b), so e.g. one XCD
 * (32 CUs) serves the cache manager and 7 XCDs keep training.  words == 0: an ordinary stream. */
int ce_stream_create_cu_mask(const uint32_t* cu_mask, int32_t words, ce_stream_t* out);
int ce_stream_destroy(ce_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Host table (the `weight` of CachedParamMgr, A.1; `pin_weight=True` at
 * benchmark/benchmark_fbgemm_uvm.py:98-105).  Pinned + device-mapped host memory.
 * ce_host_alloc pins `bytes` (first-touched by `threads` workers so a 91 GB table is
 * spread over the NUMA nodes; blocks of 64 MB and more are mapped 2 MB-aligned with
 * MADV_HUGEPAGE and then registered -- the swap workers touch one row per page -- unless
 * CE_HOST_THP=0 or the registration is refused); ce_host_register pins memory the caller already owns
 * (e.g. a `_weight` tensor).  Both return in *dev_ptr the address device code must use.
 */
int ce_host_alloc(size_t bytes, int threads, void** host_ptr, void** dev_ptr);
int ce_host_free(void* host_ptr);
int ce_host_register(void* host_ptr, size_t bytes, void** dev_ptr);
int ce_host_unregister(void* host_ptr);
/* weight init of CachedEmbeddingBag: uniform_(-1/N, 1/N) (A.7); counter-based RNG so the
 * result is independent of `threads`. */
int ce_host_fill_uniform(float* dst, int64_t n, float lo, float hi, uint64_t seed, int threads);
/* The values ce_host_fill_uniform(dst, N * dim, lo, hi, seed, .) gave the rows `rows[0..n)` of an [N, dim] table,
 * regenerated on the device into out[n, dim] (bit-identical: the generator is counter-based).  What a checker needs to
 * state "row r still holds its initial value" / "row r = initial value - lr * sum of its gradients" for a 91 GB table
 * without keeping a second copy of it. */
int ce_host_fill_uniform_rows(const int64_t* rows, int64_t n, int32_t dim, float lo, float hi, uint64_t seed,
                              float* out, ce_stream_t stream);
/* out[i] = table[rows[i]] (i < n) read through the device mapping `table_dev` of a pinned host table (the *dev_ptr of
 * ce_host_alloc / ce_host_register); rows outside [0, num_rows) give zeros.  `rows` and `out` are device memory.
 * (CachedParamMgr.cpu_weight_data for many rows at once; a PCIe-bound read.) */
int ce_host_rows_gather(const float* table_dev, int64_t num_rows, int32_t dim, const int64_t* rows, int64_t n,
                        float* out, ce_stream_t stream);
/* Memory-system probe of the box the process runs on: `reps` streaming reads, then `reps` fills, of `bytes` of
 * device scratch, each block of launches bracketed by hipEvents on `stream` (blocks until done).  A bench line carries
 * the two rates so that a reader can tell a slow box from slow code (allocations of the same GPU model differ by
 * several per cent). */
int ce_box_probe(void* scratch, size_t bytes, int32_t reps, double* read_GBps, double* fill_GBps, ce_stream_t stream);
/* How fast is THIS buffer when its rows are visited `fold` rows apart (API 5)?  The hook-folded forward stores -- and
 * the streaming backward reads -- 512-byte rows of a [B, F, D] tensor in an order that touches a different page with
 * every row (row b * F + f for consecutive b): how long that takes depends on how the allocation is mapped (the same
 * launch measures 38 or 45 us on two buffers of one process: profiles/r05_alloc_lottery.txt), not on its address or on
 * the table.  `reps` passes of row stores, then of row loads, over buf = device fp32 [rows, dim] (contents are
 * overwritten), hipEvent-bracketed on `stream`; blocks until done.  cachedembedding_amd.functional.pick_fast_buffer
 * allocates a few candidates and keeps the fastest. */
int ce_probe_rows(float* buf, int64_t rows, int32_t dim, int64_t fold, int32_t reps, double* write_us, double* read_us,
                  ce_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * K12: F.embedding_bag(slots, cuda_cached_weight, offsets, mode, per_sample_weights,
 * include_last_offset) -- reached from recsys/models/dlrm.py:99-110 and
 * benchmark/benchmark_cache.py:62 [A.7].  fp32 rows, int64 indices, int32 or int64 offsets.
 *   out[bag] = sum_j psw[j] * weight[indices[j]]   (/ len for CE_MODE_MEAN)
 * hook_features == 0: out is [num_bags, dim].  hook_features == F > 0 folds
 * sparse_embedding_shape_hook (recsys/models/dlrm.py:26-27) into the store: bags are
 * feature-major (bag = f*B + b, B = num_bags/F) and out is written as [B, F, dim].
 * include_last_offset == 0: offsets has num_bags entries and the last bag ends at nnz.
 * offsets == NULL (only with num_bags == nnz) states the one-id-per-bag layout (offsets = arange: every Criteo /
 * Avazu batch, recsys/datasets/criteo.py:127-134): the kernel then reads no offsets at all.
 */
int ce_bag_forward(const float* weight, int64_t num_rows, int32_t dim,
                   const int64_t* indices, int64_t nnz,
                   const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                   int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                   int64_t hook_features, float* out, ce_stream_t stream);

/* K13 (dense form): grad_weight[indices[j]] += psw[j]*scale*grad_out[bag(j)] accumulated into a
 * caller-zeroed [num_rows, dim] buffer -- the `sparse=False` autograd backward of K12.  Duplicates are
 * folded per 1024-lookup tile (LDS sort) before one fp32 atomic row update per (row, chunk).
 * grad_out uses the same layout convention as `out` above. */
int ce_bag_backward_dense(float* grad_weight, int64_t num_rows, int32_t dim,
                          const int64_t* indices, int64_t nnz,
                          const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                          int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                          int64_t hook_features, const float* grad_out, ce_stream_t stream);

/* K13 (sparse form): values of the COO gradient that `sparse=True` produces
 * (scripts/kaggle.sh:71 --use_sparse_embed_grad): grad_rows[j] = psw[j]*scale*grad_out[bag(j)],
 * one row per lookup, paired with `indices` as the COO indices.  dest_index (device int64[nnz],
 * NULL = identity) redirects row j to grad_rows[dest_index[j]] -- the row-wise sharded backward
 * uses it to emit the rows already in owner-bucket order. */
int ce_bag_backward_rows(float* grad_rows, const int64_t* dest_index, int32_t dim, int64_t nnz,
                         const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                         int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                         int64_t hook_features, const float* grad_out, ce_stream_t stream);

/* K13+K14 fused: weight[indices[j]] -= lr * psw[j]*scale*grad_out[bag(j)] -- autograd
 * backward + torch.optim.SGD.step on the cache parameter (recsys/dlrm_main.py:274-279,
 * 455-461) in one pass.  Same tile-sorted scatter as the dense form with alpha = -lr; the order in which
 * DIFFERENT tiles update one row is not fixed (fp32 sums may differ in the last bits run to run). */
int ce_bag_backward_sgd(float* weight, int64_t num_rows, int32_t dim,
                        const int64_t* indices, int64_t nnz,
                        const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                        int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                        int64_t hook_features, const float* grad_out, float lr, ce_stream_t stream);

/* The (row, lookup) order the backward folds duplicates in depends only on the slots, so it is computed ahead of
 * the backward, once per prefetch window on the cache-op stream right after ce_cache_prepare_ids, and over a wider
 * scope than a workgroup can sort on the fly: every SEGMENT of 16384 consecutive lookups is grouped by row (one
 * counting pass in LDS) into keys (row << 32 | lookup-in-segment, all-ones = ignored / padding, placed last).
 * ce_bag_presort handles one batch: keys_out is device uint64[ce_bag_presort_len(nnz)] (nnz rounded up to whole
 * segments).  ce_bag_presort_window handles the n_batches equal-sized batches of a window in ONE launch (indices =
 * the window's slots, batch b at [b * nnz_per_batch, (b + 1) * nnz_per_batch); keys of batch b at keys_out +
 * b * ce_bag_presort_len(nnz_per_batch); a segment never straddles two batches).
 * The *_presorted backward entry points consume the keys: same result as the unsorted forms up to fp32 summation
 * order, about half the atomic row updates. */
int64_t ce_bag_presort_len(int64_t nnz);
int ce_bag_presort(const int64_t* indices, int64_t nnz, int64_t num_rows, uint64_t* keys_out, ce_stream_t stream);
int ce_bag_presort_window(const int64_t* indices, int64_t nnz_per_batch, int64_t n_batches, int64_t num_rows,
                          uint64_t* keys_out, ce_stream_t stream);
int ce_bag_backward_sgd_presorted(float* weight, int64_t num_rows, int32_t dim,
                                  const int64_t* indices, int64_t nnz,
                                  const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                                  int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                                  int64_t hook_features, const float* grad_out, float lr,
                                  const uint64_t* presorted_keys, ce_stream_t stream);
/* the same for the plain accumulation (ce_bag_backward_dense): grad_weight += folded gradients */
int ce_bag_backward_dense_presorted(float* grad_weight, int64_t num_rows, int32_t dim,
                                    const int64_t* indices, int64_t nnz,
                                    const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                                    int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                                    int64_t hook_features, const float* grad_out,
                                    const uint64_t* presorted_keys, ce_stream_t stream);
/* Source-row keys: for mode = sum without per-sample weights every lookup scales its gradient row by the same
 * factor, so the only per-lookup facts the backward needs are the target row and WHICH row of grad_out to read.
 * ce_bag_presort_window_src resolves the second one at window time too (the bag of the lookup from the batch's
 * offsets, then its place in the [B, F, D] / [num_bags, D] output): key = row << 32 | grad_out row, same grouping
 * and layout as ce_bag_presort_window.  offsets of batch b = offsets + b * offsets_batch_stride elements (0: all
 * batches share one offsets array); num_bags / include_last_offset / hook_features describe ONE batch, as in
 * ce_bag_forward.  offsets == NULL (only with num_bags == nnz_per_batch) states the one-id-per-bag layout
 * (offsets = arange: every Criteo / Avazu batch, recsys/datasets/criteo.py:127-134) without the kernel having to read
 * the offsets to establish it.  The *_presorted_src backward entry points stream over such keys with no per-tile set-up
 * (67 vs 74 us at the bench shape); they trust the keys (grad_out row < num_bags) and ignore rows >= num_rows.
 * An ignored lookup (index outside [0, num_rows), e.g. slot -1) keeps its grad_out / output row in the low word under
 * the row 0xffffffff (API 4; all ones before) -- the backward skips it like padding, ce_bag_forward_src_keys writes its
 * zero row.
 * A lookup that NO BAG COVERS (see "Lookups that no bag covers" below) has no grad_out / output row at all: its key is
 * all ones -- row half 0xffffffff, low word 0xffffffff -- whatever its index, so every consumer skips it as it skips
 * padding (the backwards, the mark passes of the accumulator updates, and ce_bag_forward_src_keys, which writes
 * nothing for it).  Apart from those, only the positions beyond nnz_per_batch in the last segment are all ones.
 * Replaces the same upstream call as the forms above (recsys/dlrm_main.py:274-279, loss.backward + optimizer.step). */
int ce_bag_presort_window_src(const int64_t* indices, int64_t nnz_per_batch, int64_t n_batches, int64_t num_rows,
                              const void* offsets, int32_t offsets_are_i64, int64_t offsets_batch_stride,
                              int64_t num_bags, int32_t include_last_offset, int64_t hook_features,
                              uint64_t* keys_out, ce_stream_t stream);
/* K12 from the same keys, for the one-id-per-bag layout (every Criteo / Avazu batch; mode sum, no per-sample
 * weights): out[low word of key] = weight[high word of key], a zero row for an ignored lookup.  The keys are grouped by
 * row, so a cache row is LOADED once per run of equal rows and stored to every output row of the run (~50 k row loads
 * per Criteo batch instead of 425,984): the forward becomes a fill of its output instead of a copy.  `out` is
 * [nnz, dim] (or [B, F, dim] when the keys were built with hook_features = F); only valid for keys built from a layout
 * in which every bag holds exactly one lookup. */
int ce_bag_forward_src_keys(const float* weight, int64_t num_rows, int32_t dim, int64_t nnz, const uint64_t* src_keys,
                            float* out, ce_stream_t stream);
int ce_bag_backward_sgd_presorted_src(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                      const float* grad_out, float lr, const uint64_t* src_keys, ce_stream_t stream);
int ce_bag_backward_dense_presorted_src(float* grad_weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                        const float* grad_out, const uint64_t* src_keys, ce_stream_t stream);
/* Owner-exclusive form (API 3).  The fp32 atomics of the fused update retire at ~1 float per clock and L2 channel
 * (24 us for a Criteo-shaped batch, not overlapped with the gather), so rows that ONE lane group of the backward
 * can own are taken off them.  ce_bag_presort_window_src_excl additionally (a) sorts every bucket of <= 32 keys by
 * row and sets bit 31 of the low word of a key that heads a run holding ALL lookups of its row in its segment and
 * lying inside one 16-position block, and (b) records per segment the [min, max] of `ids` (device int64
 * [n_batches * nnz_per_batch], the ids `indices` was computed from, position by position; NULL = unknown) in
 * seg_id_ranges (device int64 [n_batches * segments_per_batch][2]).  ce_bag_backward_sgd_presorted_src_excl takes a
 * batch's keys and its ranges (seg_id_ranges + b * 2 * segments_per_batch): when the ranges are pairwise disjoint no
 * id -- hence no row -- occurs in two segments, a flagged run is the only writer of its row in the launch, and it is
 * applied as old row + folded gradients with one plain store; otherwise (or for unflagged runs) the atomics are
 * used, so the result never depends on the flags being usable.  Keys with flags are also valid input for the plain
 * *_presorted_src entry points (they ignore the flag). */
int ce_bag_presort_window_src_excl(const int64_t* indices, int64_t nnz_per_batch, int64_t n_batches, int64_t num_rows,
                                   const void* offsets, int32_t offsets_are_i64, int64_t offsets_batch_stride,
                                   int64_t num_bags, int32_t include_last_offset, int64_t hook_features,
                                   const int64_t* ids, uint64_t* keys_out, int64_t* seg_id_ranges,
                                   ce_stream_t stream);
int ce_bag_backward_sgd_presorted_src_excl(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                           const float* grad_out, float lr, const uint64_t* src_keys,
                                           const int64_t* seg_id_ranges, ce_stream_t stream);

/* Deterministic variant of the fused update: lookups are stably radix-sorted by target row
 * (workspace from ce_bag_backward_sgd_sorted_workspace), each row's gradients are summed in
 * lookup order and applied once:  W[r] -= lr * sum.  Matches the reference's coalesce-then-add
 * order for sparse grads; bit-reproducible, slower for very hot rows.  Lookups of rows outside
 * [0, num_rows) (the -1 of padding or of an overflowing cache call) take no part.  Lookups that
 * no bag covers (before offsets[0], or behind offsets[num_bags] with include_last_offset) take no
 * part either.  Nothing in the workspace needs initialising.
 *
 * Lookups that no bag covers -- the rule for EVERY entry that takes offsets.  Lookup j belongs to the bag b with
 * offsets[b] <= j < end(b), end(b) = offsets[b + 1], or nnz for the last bag without include_last_offset.  A lookup
 * with j < offsets[0], or j >= end(last bag) (offsets[num_bags] < nnz with include_last_offset, which torch accepts
 * and ignores the tail of), belongs to none.  The forward and ce_bag_backward_rows walk the bags and never see it;
 * the lookup-driven backwards -- ce_bag_backward_dense* / _sgd* / _rowwise_adagrad* / _update_* from slots + offsets,
 * with or without presorted keys -- skip it like a lookup outside [0, num_rows); the sorted updates skip it (above);
 * and the source-row presorts write an all-ones key for it (see ce_bag_presort_window_src).  The row it names gets no
 * gradient, no update and no momentum from it. */
size_t ce_bag_backward_sgd_sorted_workspace(int64_t num_rows, int64_t nnz);
int ce_bag_backward_sgd_sorted(float* weight, int64_t num_rows, int32_t dim,
                               const int64_t* indices, int64_t nnz,
                               const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                               int32_t include_last_offset, const float* per_sample_weights,
                               int32_t mode, int64_t hook_features, const float* grad_out, float lr,
                               void* workspace, size_t workspace_bytes, ce_stream_t stream);

/* Fused exact row-wise Adagrad (FBGEMM's EXACT_ROWWISE_ADAGRAD; weight decay: the ce_*_wd entries further down).  For every UNIQUE row of the
 * call, g = the sum of its lookups' gradient rows (as the SGD entries scale them), then
 *   momentum[m] += sum_d g[d]^2 / dim ;  weight[slot] -= lr * g / (sqrt(momentum[m]) + eps)
 * with m = row_of_slot[slot] (row_of_slot: device int32[num_rows], the cache's cached_idx_map; NULL = the slot itself)
 * and momentum device fp32[momentum_rows]; a slot whose m lies outside [0, momentum_rows) is not updated.  Lookups of
 * rows outside [0, num_rows) are ignored.  The workspace (device, 256-byte aligned, at least
 * ce_bag_backward_rowwise_adagrad_workspace(num_rows, dim) bytes) must be ZERO-FILLED before its first use; every call
 * leaves it zero-filled again.  No host synchronisation, no allocation: the calls can be captured into a hipGraph.
 * The general form takes slots + offsets (sum / mean, per-sample weights, hook_features; presorted: optional keys
 * from ce_bag_presort* as for ce_bag_backward_dense_presorted); the _src form takes a batch's source-row keys
 * (ce_bag_presort_window_src*). */
size_t ce_bag_backward_rowwise_adagrad_workspace(int64_t num_rows, int32_t dim);
int ce_bag_backward_rowwise_adagrad(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices, int64_t nnz,
                                    const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                                    int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                                    int64_t hook_features, const float* grad_out, const uint64_t* presorted,
                                    const int32_t* row_of_slot, float* momentum, int64_t momentum_rows, float lr,
                                    float eps, void* workspace, size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_rowwise_adagrad_src(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                        const float* grad_out, const uint64_t* src_keys, const int32_t* row_of_slot,
                                        float* momentum, int64_t momentum_rows, float lr, float eps, void* workspace,
                                        size_t workspace_bytes, ce_stream_t stream);

/* Half-precision activations (additions to API 6).  The entries below are the hot-path entries above with the
 * pooled output / the incoming gradient as `void*` of act_dtype (CE_ACT_F32 / CE_ACT_BF16 / CE_ACT_F16) -- fp32
 * weight, fp32 accumulation, ONE rounding on the forward's store, an exact upcast on the backward's gather; the 16-bit
 * tensor is read / written by the kernel itself (no staging tensor, no extra launch, capture-safe as their fp32
 * forms).  With CE_ACT_F32 each is its fp32 form, which now forwards here.  Fewer entries than there: `presorted_keys`
 * (NULL = the kernel sorts its own tiles) merges ce_bag_backward_{dense,sgd} with their _presorted forms, and
 * `seg_id_ranges` (NULL = atomics everywhere) merges ce_bag_backward_sgd_presorted_src with its _excl form.
 * A 16-bit tensor must be 2-byte aligned; 8-byte aligned with dim % 4 == 0 takes the vector kernels (a lane moves its
 * 4 elements as 8 bytes: dim = 20 or 100 qualify), anything else the scalar ones (dim <= 256).  The two key-driven
 * kernels (ce_bag_forward_src_keys_act, the _src_act backwards) move 16 bytes per lane -- two keys per lane pair --
 * when dim % 8 == 0 and the tensor is 16-byte aligned (what torch allocates).  An unknown act_dtype
 * returns CE_ERR_INVALID and launches nothing.  Off the hot path (ce_bag_forward_max, ce_bag_backward_max / _psw /
 * _rows / _sgd_sorted) there is no _act form: a caller converts. */
int ce_bag_forward_act(const float* weight, int64_t num_rows, int32_t dim,
                       const int64_t* indices, int64_t nnz,
                       const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                       int32_t include_last_offset, const float* per_sample_weights,
                       int32_t mode, int64_t hook_features, void* out, int32_t act_dtype, ce_stream_t stream);
int ce_bag_forward_src_keys_act(const float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                const uint64_t* src_keys, void* out, int32_t act_dtype, ce_stream_t stream);
int ce_bag_backward_dense_act(float* grad_weight, int64_t num_rows, int32_t dim,
                              const int64_t* indices, int64_t nnz,
                              const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                              int32_t include_last_offset, const float* per_sample_weights,
                              int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                              const uint64_t* presorted_keys, ce_stream_t stream);
int ce_bag_backward_sgd_act(float* weight, int64_t num_rows, int32_t dim,
                            const int64_t* indices, int64_t nnz,
                            const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                            int32_t include_last_offset, const float* per_sample_weights,
                            int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype, float lr,
                            const uint64_t* presorted_keys, ce_stream_t stream);
int ce_bag_backward_sgd_src_act(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                const void* grad_out, int32_t act_dtype, float lr, const uint64_t* src_keys,
                                const int64_t* seg_id_ranges, ce_stream_t stream);
int ce_bag_backward_dense_src_act(float* grad_weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                  const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                  ce_stream_t stream);
int ce_bag_backward_rowwise_adagrad_act(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices,
                                        int64_t nnz, const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                                        int32_t include_last_offset, const float* per_sample_weights, int32_t mode,
                                        int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                        const uint64_t* presorted, const int32_t* row_of_slot, float* momentum,
                                        int64_t momentum_rows, float lr, float eps, void* workspace,
                                        size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_rowwise_adagrad_src_act(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                            const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                            const int32_t* row_of_slot, float* momentum, int64_t momentum_rows,
                                            float lr, float eps, void* workspace, size_t workspace_bytes,
                                            ce_stream_t stream);

/* 16-bit table (additions to API 6).  The TABLE's rows are bf16 / fp16: weight_dtype = CE_ACT_BF16 / CE_ACT_F16
 * (CE_ACT_F32 and unknown codes: CE_ERR_INVALID before any launch).  dim % 8 == 0 and dim <= 1024 -- rows are whole
 * 16-byte units, so a [N, dim] 16-bit table has the bytes of an fp32 [N, dim / 2] table and the cache op, which only
 * moves rows, is driven with embedding_dim = dim / 2 -- and the table 16-byte aligned; any other dim is
 * CE_ERR_UNSUPPORTED before any launch.  Rows are up-converted exactly on load and summed in fp32; the forward rounds
 * once, on the store to act_dtype.  ce_bag_forward_src_keys_w16 with act_dtype == weight_dtype copies the row's bits
 * (nothing is rounded or canonicalised; an ignored lookup's output row is zero).
 *
 * The update: fp32 atomics cannot land on 16-bit rows, so the step's gradient is folded into an fp32 accumulator first
 * and the row is rounded ONCE, after its whole gradient is known.  Three launches, no host synchronisation, no
 * allocation (capture-safe): mark the looked-up slots (one thread also adds 1 to the step counter), the dense backward
 * (ce_bag_backward_dense_act / _dense_src_act) into acc[slot], then one apply pass over the flagged slots:
 *   CE_OPT_SGD:             x = w - lr * g                                  (row_of_slot / momentum may be NULL, eps ignored)
 *   CE_OPT_ROWWISE_ADAGRAD: m[row] += sum_d g[d]^2 / dim ;  x = w - lr * g / (sqrt(m[row]) + eps)
 *   W16[slot] = round(x), acc[slot] = 0, flag = 0       (w = the exact up-conversion of the old row, all in fp32)
 * CE_ROUND_NEAREST: the plain cast (round-to-nearest-even, NaN kept).  CE_ROUND_STOCHASTIC: one of the two 16-bit
 * neighbours of x (x itself when representable), the one farther from zero with probability (distance to the nearer
 * one) / (their spacing); NaN, infinities, fp16 results below 2^-14 or from 65504 on, and bf16 values beyond the largest
 * finite one take the nearest cast.  The random bits are a counter-based hash of (seed, step counter, row_of_slot[slot]
 * or the slot when NULL, element): independent of the slot a row sits in, of the grid and of timing; a replayed graph
 * draws fresh bits each step because the counter lives in the workspace.
 * Workspace (ce_bag_backward_w16_workspace bytes, 256-byte aligned): fp32 acc [num_rows, dim], byte flags [num_rows],
 * one 64-bit step counter.  Zero-filled by its owner once; every call leaves it zero-filled except the counter, which
 * counts the calls.  Everything the entries can refuse is refused before the first launch. */
#define CE_OPT_SGD 0
#define CE_OPT_ROWWISE_ADAGRAD 1
#define CE_ROUND_NEAREST 0
#define CE_ROUND_STOCHASTIC 1
/* element i = the round-to-nearest-even cast to `dtype` (CE_ACT_BF16 / CE_ACT_F16) of what ce_host_fill_uniform writes
 * at element i for the same arguments */
int ce_host_fill_uniform_w16(void* dst, int64_t n, float lo, float hi, uint64_t seed, int32_t dtype, int threads);
int ce_bag_forward_w16(const void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                       const int64_t* indices, int64_t nnz,
                       const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                       int32_t include_last_offset, const float* per_sample_weights,
                       int32_t mode, int64_t hook_features, void* out, int32_t act_dtype, ce_stream_t stream);
int ce_bag_forward_src_keys_w16(const void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim, int64_t nnz,
                                const uint64_t* src_keys, void* out, int32_t act_dtype, ce_stream_t stream);
size_t ce_bag_backward_w16_workspace(int64_t num_rows, int32_t dim);
int ce_bag_backward_update_w16(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                               const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                               int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                               int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                               const uint64_t* presorted, const int32_t* row_of_slot, float* momentum,
                               int64_t momentum_rows, float lr, float eps, int32_t optimizer, int32_t rounding,
                               uint64_t seed, void* workspace, size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_update_src_w16(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim, int64_t nnz,
                                   const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                   const int32_t* row_of_slot, float* momentum, int64_t momentum_rows, float lr,
                                   float eps, int32_t optimizer, int32_t rounding, uint64_t seed, void* workspace,
                                   size_t workspace_bytes, ce_stream_t stream);

/* Deterministic, accumulator-free fused update (additions to API 6): the update of the entries above -- row-wise
 * Adagrad or SGD, on an fp32 (weight_dtype = CE_ACT_F32), bf16 or fp16 table, grad_out read in place as act_dtype --
 * with a bit-reproducible gradient fold and a workspace proportional to the LOOKUPS, not to the table.
 * The lookups are stably radix-sorted by row, so a row's lookups form a run in ascending lookup position.  Fold order:
 *   - a run of n <= CE_SORTED_CHUNK lookups: g = (...((s_0 g_0) + s_1 g_1) + ...) in fp32, strictly in lookup order
 *     (s_j: per-sample weight, 1 / len for mean; for s_j == 1 the term is the gradient row itself);
 *   - a longer run is cut into chunks of CE_SORTED_CHUNK consecutive positions counted from the start of the run, each
 *     chunk is folded sequentially from zero by a lane group of its own, and the partial sums are added in ascending
 *     chunk order.
 * The result depends on the batch alone -- not on the grid, on the slot a row sits in, or on timing.  The row is then
 * updated once, with the arithmetic of ce_bag_backward_rowwise_adagrad* / ce_bag_backward_update_w16: a row looked up
 * once gets the same bits on either path.  The term s_j g_j is rounded to fp32 before it is added (no fused
 * multiply-add).  A 16-bit row is stored with CE_ROUND_NEAREST; CE_ROUND_STOCHASTIC on a 16-bit table is refused
 * (CE_ERR_UNSUPPORTED).  `rounding` is ignored for an fp32 table; `seed`, which only stochastic rounding would read,
 * is ignored.
 * Lookups outside [0, num_rows) (the -1 of padding) take no part; a slot whose momentum index lies outside
 * [0, momentum_rows) is not updated.  CE_OPT_SGD: row_of_slot / momentum may be NULL, eps is ignored.
 * Workspace: ce_bag_backward_update_sorted_workspace bytes (independent of num_rows), 256-byte aligned: the sort arrays
 * (5 int32 per lookup + the digit histograms), then 2 * ceil(nnz / CE_SORTED_CHUNK) fp32 partial rows.  Nothing in it
 * needs initialising and nothing in it outlives the call (no step counter: without stochastic rounding no state passes
 * from one call to the next).  No host synchronisation, no allocation, launch shapes fixed by the arguments
 * (capture-safe).  Everything that can be refused -- null pointers, sizes beyond 2^31, unknown dtype / optimizer /
 * rounding codes, stochastic rounding, a 16-bit table's dim rule or alignment, a workspace that is too small -- is
 * refused before the first launch.
 * The tables that carry their state in the row (Adam, partial row-wise Adam, element-wise Adagrad) have this fold in
 * entries of their own: ce_bag_backward_adam_sorted / _pradam_sorted / _adagrad_sorted, further down. */
#define CE_SORTED_CHUNK 64
size_t ce_bag_backward_update_sorted_workspace(int64_t num_rows, int64_t nnz, int32_t dim);
int ce_bag_backward_update_sorted(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                  const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                                  int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                                  int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                  const int32_t* row_of_slot, float* momentum, int64_t momentum_rows, float lr, float eps,
                                  int32_t optimizer, int32_t rounding, uint64_t seed, void* workspace,
                                  size_t workspace_bytes, ce_stream_t stream);

/* Step-sized accumulator for the atomic fused updates (additions to API 6): the update of ce_bag_backward_rowwise_adagrad*
 * (weight_dtype = CE_ACT_F32, CE_OPT_ROWWISE_ADAGRAD) and of ce_bag_backward_update_w16 / _src_w16 (bf16 / fp16 table,
 * either optimizer) with an fp32 accumulator of cap = min(nnz, num_rows) rows instead of num_rows: a step cannot touch
 * more distinct slots than it has lookups.  The argument lists are those of the _w16 entries.  One stream, no host
 * synchronisation, no allocation, launch shapes fixed by the arguments (capture-safe):
 *   mark (as above: byte flags, the 16-bit table's step counter) -> an ordered compaction of the flagged slots
 *   (list[u] = the u-th flagged slot ascending, cidx[slot] = u, their number U; the flags return to zero) -> one
 *   elementwise pass that rewrites the slots / the row half of the keys as cidx[.] into the workspace (lookups outside
 *   [0, num_rows) -> -1, ignored rows and padding keys stay) -> the same dense backward into acc[cap, dim] ->
 *   one apply pass over u < U that updates W[list[u]] and momentum[row_of_slot[list[u]]] and zeroes acc[u].
 * Given the same folded gradient the apply pass writes the bits of the entries above, stochastic rounding of an SGD step
 * included (same hash of seed, step counter, row and element).
 * CE_ERR_UNSUPPORTED before the first launch: CE_OPT_SGD on an fp32 table (it has no accumulator), and row-wise Adagrad
 * with CE_ROUND_STOCHASTIC on a 16-bit table.  `rounding` and `seed` are ignored for an fp32 table.  Every other refusal
 * is that of the entries above, from the arguments alone.
 * Workspace: ce_bag_backward_update_compact_workspace(num_rows, nnz, dim) bytes, 256-byte aligned, at most
 * 6 * num_rows + cap * (4 * dim + 4) + 8 * ce_bag_presort_len(nnz) + 65536 -- nothing in it is proportional to
 * num_rows * dim.  In order, each part padded to 256 bytes: the 64-bit step counter, U, byte flags [num_rows], fp32 acc
 * [cap, dim], then cidx, the scan's counts (one per CE_COMPACT_BLOCK slots), list and the rewritten slots / keys.  Zero-filled
 * by its owner once; every call leaves the counter counting the calls, the flags and acc zero; the rest needs no
 * initialising.  The layout depends on (num_rows, nnz, dim): before a workspace serves another triple its owner
 * zero-fills it again (the counter may be kept). */
#define CE_COMPACT_BLOCK 4096
size_t ce_bag_backward_update_compact_workspace(int64_t num_rows, int64_t nnz, int32_t dim);
int ce_bag_backward_update_compact(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                   const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                                   int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                                   int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                   const uint64_t* presorted, const int32_t* row_of_slot, float* momentum,
                                   int64_t momentum_rows, float lr, float eps, int32_t optimizer, int32_t rounding,
                                   uint64_t seed, void* workspace, size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_update_compact_src(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim, int64_t nnz,
                                       const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                       const int32_t* row_of_slot, float* momentum, int64_t momentum_rows, float lr,
                                       float eps, int32_t optimizer, int32_t rounding, uint64_t seed, void* workspace,
                                       size_t workspace_bytes, ce_stream_t stream);

/* Learning rate from device memory for the atomic fused updates (additions to API 6).  Every fused update above takes
 * `float lr`; a hipGraph capture freezes that float, so a replayed step cannot follow a learning-rate schedule.  The
 * four entries below are existing argument lists with `float lr` replaced by `const float* lr`:
 *   ce_bag_backward_sgd_lrdev        the list of ce_bag_backward_sgd_act     (fp32 table, slots + offsets, optional keys)
 *   ce_bag_backward_sgd_src_lrdev    the list of ce_bag_backward_sgd_src_act (source-row keys, optional seg_id_ranges)
 *   ce_bag_backward_update_lrdev     the list of ce_bag_backward_update_w16 plus `accumulator` behind `seed`; it covers
 *                                      CE_ACC_CACHE, CE_ACT_F32 table : ce_bag_backward_rowwise_adagrad_act
 *                                      CE_ACC_CACHE, 16-bit table     : ce_bag_backward_update_w16
 *                                      CE_ACC_STEP                    : ce_bag_backward_update_compact
 *   ce_bag_backward_update_src_lrdev the same from source-row keys: ce_bag_backward_rowwise_adagrad_src_act,
 *                                    ce_bag_backward_update_src_w16, ce_bag_backward_update_compact_src
 * The workspace is the one the covered entry takes for that accumulator and table type (ce_bag_backward_rowwise_adagrad_
 * workspace, ce_bag_backward_w16_workspace, ce_bag_backward_update_compact_workspace).
 *   - `lr` points to ONE fp32 in device memory, 4-byte aligned.
 *   - The kernels of the call read it when they RUN (once per thread, at the top of the kernel): a stream-ordered write
 *     before the call counts, and a replayed graph reads the value of the moment of the replay.
 *   - Nothing on the host reads the value: no synchronisation, no allocation.  The launch shapes are those of the
 *     by-value sibling, so the entry is capture-safe as that one is.
 *   - With *lr == v the entry writes the bits the by-value sibling writes for lr = v: weights, momentum and the
 *     stochastic rounding bits (the SGD scatter scales by -(*lr), a negation; the apply pass is the same update_row).
 *   - The host cannot check the value.  The by-value update entries refuse lr < 0; here a negative or NaN value takes
 *     part in the arithmetic as it is.
 *   - lr == NULL is CE_ERR_INVALID ("lr: null device pointer") before the first launch, and it is the FIRST check of
 *     the entry: it comes before every refusal of the sibling, also for a call the sibling returns from at once
 *     (nnz == 0).  In the two update entries an unknown accumulator code is the second check (CE_ERR_INVALID).
 *   - Every other refusal has the sibling's code, message and position in the order of checks; the by-value entry and
 *     this one are the same function, called with and without the pointer.
 *   - The update entries refuse what the covered entry refuses: CE_OPT_SGD on an fp32 table (CE_ERR_UNSUPPORTED with
 *     either accumulator, where the sibling's not-taken check stands: the two sgd entries above are that update),
 *     row-wise Adagrad with CE_ROUND_STOCHASTIC on a 16-bit table with CE_ACC_STEP, and everything else.  With
 *     CE_ACC_CACHE on an fp32 table `rounding` and `seed` are not looked at (the covered entry has neither).
 * Not covered: the sorted, deterministic updates (ce_bag_backward_sgd_sorted, ce_bag_backward_update_sorted),
 * ce_bag_backward_max and ce_rows_axpy keep `float lr` / `float alpha` only. */
#define CE_ACC_CACHE 0
#define CE_ACC_STEP 1
int ce_bag_backward_sgd_lrdev(float* weight, int64_t num_rows, int32_t dim,
                              const int64_t* indices, int64_t nnz,
                              const void* offsets, int32_t offsets_are_i64, int64_t num_bags,
                              int32_t include_last_offset, const float* per_sample_weights,
                              int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                              const float* lr, const uint64_t* presorted_keys, ce_stream_t stream);
int ce_bag_backward_sgd_src_lrdev(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                  const void* grad_out, int32_t act_dtype, const float* lr, const uint64_t* src_keys,
                                  const int64_t* seg_id_ranges, ce_stream_t stream);
int ce_bag_backward_update_lrdev(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                 const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                                 int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                                 int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                 const uint64_t* presorted, const int32_t* row_of_slot, float* momentum,
                                 int64_t momentum_rows, const float* lr, float eps, int32_t optimizer, int32_t rounding,
                                 uint64_t seed, int32_t accumulator, void* workspace, size_t workspace_bytes,
                                 ce_stream_t stream);
int ce_bag_backward_update_src_lrdev(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim, int64_t nnz,
                                     const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                     const int32_t* row_of_slot, float* momentum, int64_t momentum_rows,
                                     const float* lr, float eps, int32_t optimizer, int32_t rounding, uint64_t seed,
                                     int32_t accumulator, void* workspace, size_t workspace_bytes, ce_stream_t stream);

/* Fused Adam with the moments carried in the row, layout `adam` (additions to API 6).  Adam's two moments are as large
 * as the table, so they cannot stay in HBM beside a cache of 1 % of it: they live where the table lives and travel
 * with the rows.  An fp32 table only.  A row of `dim` elements is 3 * dim floats:
 *   w[0 .. dim) | m[dim .. 2 dim) | v[2 dim .. 3 dim)        (weights, first moment, second moment)
 * dim % 4 == 0, 4 <= dim <= 1024 and the table 16-byte aligned, so all three parts of every row start on a 16-byte
 * boundary and only the vector lane form exists (the cache op, which only moves rows, is driven with embedding_dim =
 * 3 * dim: the moments survive eviction and admission with no cache kernel knowing of them).  Any other dim:
 * CE_ERR_UNSUPPORTED before any launch.  `weight` is [num_rows, 3 * dim] in every entry below; `dim` stays D.
 *
 * ce_host_fill_uniform_adam: row r's w part = what ce_host_fill_uniform gives row r of an [n_rows, dim] table for the
 * same (lo, hi, seed) -- element r * dim + d of that fill --, its moments zero.  Host memory, no GPU; the result does
 * not depend on `threads`.
 *
 * The two forwards are ce_bag_forward_act / ce_bag_forward_src_keys_act in every respect but the row type (the same
 * kernels with a row stride of three rows' width): they read the w part alone -- sum / mean, per-sample weights,
 * hook_features, int32 / int64 / NULL offsets, act_dtype, a zero row for an ignored key; capture-safe; the dim rule,
 * then null pointers, then misalignment (the table 16 bytes, `out` its vector boundary) are refused before the first
 * launch.  The result is bit-equal to the fp32 sibling's over a contiguous copy of the w parts.
 *
 * ce_bag_backward_adam (slots + offsets, optional segment-sorted keys) and ce_bag_backward_adam_src (source-row keys)
 * take the lists of ce_bag_backward_update_lrdev / _src_lrdev without weight_dtype, row_of_slot, momentum,
 * momentum_rows, optimizer, rounding and seed, and with beta1, beta2, `float lr` TOGETHER WITH `const float* lr_dev`,
 * and `int64_t* step`.
 *   - lr_dev == NULL: the learning rate is `lr`.  Otherwise it points to ONE fp32 in device memory that the kernels
 *     read when they run, as the ce_*_lrdev entries read theirs, and `lr` is ignored.
 *   - `step` is ONE int64 in device memory, 8-byte aligned, owned by the caller (zero before the first step).  The
 *     first launch of a call adds 1 to it; t below is its value after that.  It lives outside the workspace so that it
 *     outlives it, and on the device so that a replayed graph counts on.
 *   - accumulator: CE_ACC_CACHE -- the pipeline of ce_bag_backward_rowwise_adagrad* (mark, the dense backward into
 *     acc[num_rows, dim], one apply pass over the flags) -- or CE_ACC_STEP -- that of ce_bag_backward_update_compact*
 *     (mark, compaction, rewrite, the dense backward into acc[min(nnz, num_rows), dim], one apply pass over the list).
 *     Workspace: ce_bag_backward_adam_workspace(num_rows, nnz, dim, accumulator) bytes = what
 *     ce_bag_backward_rowwise_adagrad_workspace(num_rows, dim) / ce_bag_backward_update_compact_workspace(num_rows,
 *     nnz, dim) return, 256-byte aligned, with the same contract: zero-filled by its owner once, left zero-filled by
 *     every call (the step-sized one: flags and acc; its own counter is not used).
 *   - The arithmetic is torch.optim.SparseAdam's, every operation rounded on its own (no contraction).  For every
 *     UNIQUE row the call looks up, g its folded gradient of the call:
 *         omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2)                       (fp64 difference, rounded)
 *         c_t  = (float)(sqrt(1.0 - pow(beta2, t)) / (1.0 - pow(beta1, t)))              (fp64, on the device)
 *         m' = m + omb1 * (g - m) ;  v' = v + omb2 * (g * g - v) ;  w' = w - (lr * c_t) * (m' / (sqrtf(v') + eps))
 *     Rows no lookup names keep w, m and v bit for bit.  Lookups outside [0, num_rows) and lookups no bag covers take
 *     no part ("Lookups that no bag covers" above) -- the mark pass skips them too, because here a row that is merely
 *     flagged changes.  A row named only by zero-weight lookups has g = 0 and still decays its moments, as in torch.
 *     Given the same folded gradient both accumulators write the same bits (one update_row).
 *   - No host synchronisation, no allocation, launch shapes fixed by the arguments (capture-safe).
 *   - Refused before the first launch, in this order: step == NULL (CE_ERR_INVALID; the first check), an unknown
 *     accumulator, a beta outside [0, 1), eps < 0, a by-value lr < 0 (or NaN), an unknown act_dtype, the dim rule
 *     (CE_ERR_UNSUPPORTED), null pointers and sizes beyond 2^31, misalignment (table 16 bytes, step 8, workspace 256),
 *     a workspace that is too small; then, for a call with lookups, what the covered pipeline refuses (null indices /
 *     offsets / keys, mean with per-sample weights, hook_features that does not divide num_bags).
 *   - nnz == 0 (or num_bags == 0) returns after those checks with no launch: it does not count a step.
 * Not built: 16-bit moments or tables.  The sorted (deterministic) fold: ce_bag_backward_adam_sorted below.  Weight decay (L2 as torch.optim.Adam's,
 * decoupled as torch.optim.AdamW's): ce_bag_backward_adam_wd / _adam_src_wd below. */
int ce_host_fill_uniform_adam(float* dst, int64_t n_rows, int32_t dim, float lo, float hi, uint64_t seed, int threads);
int ce_bag_forward_adam(const float* weight, int64_t num_rows, int32_t dim,
                        const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                        int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                        int32_t mode, int64_t hook_features, void* out, int32_t act_dtype, ce_stream_t stream);
int ce_bag_forward_src_keys_adam(const float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                 const uint64_t* src_keys, void* out, int32_t act_dtype, ce_stream_t stream);
size_t ce_bag_backward_adam_workspace(int64_t num_rows, int64_t nnz, int32_t dim, int32_t accumulator);
int ce_bag_backward_adam(float* weight, int64_t num_rows, int32_t dim,
                         const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                         int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                         int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                         const uint64_t* presorted, double beta1, double beta2, float lr, const float* lr_dev,
                         float eps, int64_t* step, int32_t accumulator, void* workspace, size_t workspace_bytes,
                         ce_stream_t stream);
int ce_bag_backward_adam_src(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                             const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                             double beta1, double beta2, float lr, const float* lr_dev, float eps, int64_t* step,
                             int32_t accumulator, void* workspace, size_t workspace_bytes, ce_stream_t stream);

/* Weight decay for the fused updates (additions to API 6): L2 and decoupled, lazy.  Five entries; each is an existing
 * argument list with `float weight_decay, int32_t weight_decay_mode` directly behind `eps`:
 *   ce_bag_backward_update_wd        the list of ce_bag_backward_update_lrdev with `float lr, const float* lr_dev` in
 *                                    place of `const float* lr` (Adam's convention: lr_dev == NULL means by value):
 *                                    row-wise Adagrad on fp32 / bf16 / fp16 tables, SGD on 16-bit tables, CE_ACC_CACHE
 *                                    and CE_ACC_STEP
 *   ce_bag_backward_update_src_wd    the same from source-row keys (the list of ce_bag_backward_update_src_lrdev)
 *   ce_bag_backward_update_sorted_wd the list of ce_bag_backward_update_sorted (float lr only): the deterministic fold,
 *                                    Adagrad and SGD, fp32 and 16-bit tables with CE_ROUND_NEAREST
 *   ce_bag_backward_adam_wd          the list of ce_bag_backward_adam (Adam-layout table, both accumulators)
 *   ce_bag_backward_adam_src_wd      the list of ce_bag_backward_adam_src
 * The workspaces are those of the covered entries, with the same contracts; so are the refusals, their codes, messages
 * and order, capture-safety, no host synchronisation, no allocation.
 *
 * The decay is LAZY, as FBGEMM's and torch.optim.SparseAdam's state updates are: in a call exactly the rows the call
 * NAMES are decayed, once, however often they are named.  A row is named if some lookup that a bag covers has its slot
 * in [0, num_rows) (a source-row key: a row half below num_rows).  A row named only by zero-weight lookups (g = 0) still
 * decays; rows no covered lookup names keep their bits -- w, momentum and moments.  (So the mark pass of the slots +
 * offsets forms flags covered lookups only here, and the sorted form gives uncovered lookups the ignored key.)
 * All arithmetic is fp32 with contraction off, every operation rounded on its own.  w: the row before the call (a 16-bit
 * row up-converted exactly), g: its folded gradient:
 *   CE_WD_L2        (torch.optim.{SGD, Adagrad, Adam}(weight_decay=), FBGEMM L2):  h = g + wd * w per element (the
 *                   product rounded, then the sum); the covered entry's update with h in place of g EVERYWHERE: row-wise
 *                   Adagrad's sum h^2 / dim, the momentum and the step; Adam's m' and v'; SGD's w - lr * h.
 *   CE_WD_DECOUPLED (torch.optim.AdamW, FBGEMM DECOUPLE):  f = (float)(1.0 - (double)lr * (double)wd), lr the call's
 *                   learning rate -- *lr_dev when that is given, read when the kernels run, so a replayed graph follows
 *                   a schedule in the decay too; for Adam lr, not lr * c_t --;  w_d = w * f per element; the covered
 *                   entry's update with w_d in place of w and the raw g.
 *   CE_WD_NONE, or weight_decay == 0 with any mode: the covered entry's update, by the covered entry's kernels: the
 *                   bits are those of the covered entry.
 * Row-wise Adagrad: a slot whose momentum index lies outside [0, momentum_rows) is not touched, so it does not decay.
 * A 16-bit row is rounded once per call, nearest or stochastic (same hash of seed, step counter, row and element).
 * A row looked up once in a call gets the same bits from CE_ACC_CACHE, CE_ACC_STEP and the sorted entry.
 * Refusals: an unknown weight_decay_mode, then a weight_decay that is negative or NaN, are CE_ERR_INVALID.  The two
 * checks stand directly behind the entry's leading checks -- the accumulator code in the update entries; step == NULL
 * and the accumulator code in the Adam entries; nothing in the sorted entry, where they come first -- before every
 * other refusal, and also for nnz == 0.  CE_OPT_SGD on an fp32 table stays CE_ERR_UNSUPPORTED in the two atomic entries
 * (that scatter has no per-row pass): fp32 SGD with decay exists through the sorted entry only.
 * Not built: FBGEMM's COUNTER / COWCLIP modes, a decay read from device memory, decay in ce_rows_axpy. */
#define CE_WD_NONE 0
#define CE_WD_L2 1
#define CE_WD_DECOUPLED 2
int ce_bag_backward_update_wd(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                              const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                              int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                              int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                              const uint64_t* presorted, const int32_t* row_of_slot, float* momentum,
                              int64_t momentum_rows, float lr, const float* lr_dev, float eps, float weight_decay,
                              int32_t weight_decay_mode, int32_t optimizer, int32_t rounding, uint64_t seed,
                              int32_t accumulator, void* workspace, size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_update_src_wd(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim, int64_t nnz,
                                  const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                  const int32_t* row_of_slot, float* momentum, int64_t momentum_rows, float lr,
                                  const float* lr_dev, float eps, float weight_decay, int32_t weight_decay_mode,
                                  int32_t optimizer, int32_t rounding, uint64_t seed, int32_t accumulator,
                                  void* workspace, size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_update_sorted_wd(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                     const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                                     int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                                     int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                     const int32_t* row_of_slot, float* momentum, int64_t momentum_rows, float lr,
                                     float eps, float weight_decay, int32_t weight_decay_mode, int32_t optimizer,
                                     int32_t rounding, uint64_t seed, void* workspace, size_t workspace_bytes,
                                     ce_stream_t stream);
int ce_bag_backward_adam_wd(float* weight, int64_t num_rows, int32_t dim,
                            const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                            int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                            int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                            const uint64_t* presorted, double beta1, double beta2, float lr, const float* lr_dev,
                            float eps, float weight_decay, int32_t weight_decay_mode, int64_t* step,
                            int32_t accumulator, void* workspace, size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_adam_src_wd(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                double beta1, double beta2, float lr, const float* lr_dev, float eps,
                                float weight_decay, int32_t weight_decay_mode, int64_t* step, int32_t accumulator,
                                void* workspace, size_t workspace_bytes, ce_stream_t stream);

/* Partial row-wise Adam, layout `partial_rowwise_adam` (additions to API 6; FBGEMM's PARTIAL_ROWWISE_ADAM).  The first
 * moment is kept per element and travels in the row, as in the Adam layout; the second moment is ONE fp32 per table
 * row, fed by the mean of the row's squared gradient, and stays in device memory where row-wise Adagrad keeps its
 * momentum.  An fp32 table only.  A row of `dim` elements is 2 * dim floats:
 *   w[0 .. dim) | m[dim .. 2 dim)                             (weights, first moment)
 * The dim rule and the alignment are the Adam layout's (dim % 4 == 0, 4 <= dim <= 1024, the table 16-byte aligned;
 * vector lanes only; the cache op is driven with embedding_dim = 2 * dim).  `weight` is [num_rows, 2 * dim] in every
 * entry below; `dim` stays D.
 *
 * ce_host_fill_uniform_pradam is ce_host_fill_uniform_adam for rows of 2 * dim floats: the same w parts, a zero m.
 *
 * ce_bag_forward_pradam / ce_bag_forward_src_keys_pradam are ce_bag_forward_adam / _src_keys_adam with a row stride of
 * two rows' width: they read the w part alone, the result is bit-equal to the fp32 sibling's over a contiguous copy
 * of the w parts, the refusals and their order are the same.  No PAIR form.
 *
 * ce_bag_backward_pradam / ce_bag_backward_pradam_src take the lists of ce_bag_backward_adam_wd / _adam_src_wd with
 * `const int32_t* row_of_slot, float* v, int64_t v_rows` directly before beta1 -- the three arguments row-wise Adagrad
 * calls row_of_slot, momentum, momentum_rows: v is [v_rows] fp32 in device memory, indexed by r = row_of_slot[s] for
 * the row in slot s (row_of_slot == NULL: r = s), zero before the first step, never moved by the cache.  lr / lr_dev,
 * `step`, the accumulators, the workspace (ce_bag_backward_pradam_workspace = ce_bag_backward_adam_workspace), the
 * decay (weight_decay_mode CE_WD_NONE or weight_decay == 0: the instantiations without decay) and capture safety are
 * those entries'.  The arithmetic, every operation rounded on its own (no contraction), for every UNIQUE row the call
 * looks up, in slot s, g its folded gradient of the call, t the step count after the call's first launch:
 *     omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2)                         (fp64 difference, rounded)
 *     c_t  = (float)(sqrt(1.0 - pow(beta2, t)) / (1.0 - pow(beta1, t)))                (fp64, on the device)
 *     h  = g                                                                            no decay
 *     h  = g + weight_decay * w                                                         CE_WD_L2
 *     w  = w * f, h = g ; f = (float)(1.0 - (double)lr * (double)weight_decay)          CE_WD_DECOUPLED
 *     ss = sum of h_i^2 over the row: per lane as row-wise Adagrad's fp32 table sums it (the lane's last chunk
 *          ((x^2 + y^2) + z^2) + w^2, the chunks before it fma chains, added in chunk order), then the xor tree across
 *          the row's lane group, widest stride first
 *     v' = v[r] + omb2 * (ss / D - v[r])                                                one scalar; lane 0 stores it
 *     m' = m + omb1 * (h - m)                                                           per element
 *     w' = w - (lr * c_t) * (m' / (sqrtf(v') + eps))                                    per element
 *   - r outside [0, v_rows): nothing happens to the slot -- w and m keep their bits, no decay either (row-wise
 *     Adagrad's rule).  Rows no lookup names keep w, m and v[r] bit for bit.  Lookups outside [0, num_rows) and
 *     lookups no bag covers take no part and flag nothing.  A row named only by zero-weight lookups has g = 0 and
 *     still decays m and v.  Given the same folded gradient both accumulators write the same bits.
 *   - Refused before the first launch: what ce_bag_backward_adam_wd refuses, in its order, and v == NULL or
 *     v_rows <= 0 (CE_ERR_INVALID) directly behind its null-pointer check.  nnz == 0 (or num_bags == 0) returns after
 *     the checks with no launch: it does not count a step.
 * Not built: 16-bit moments or tables, a scalar lane form.  (The sorted fold: ce_bag_backward_pradam_sorted.) */
int ce_host_fill_uniform_pradam(float* dst, int64_t n_rows, int32_t dim, float lo, float hi, uint64_t seed, int threads);
int ce_bag_forward_pradam(const float* weight, int64_t num_rows, int32_t dim,
                          const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                          int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                          int32_t mode, int64_t hook_features, void* out, int32_t act_dtype, ce_stream_t stream);
int ce_bag_forward_src_keys_pradam(const float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                   const uint64_t* src_keys, void* out, int32_t act_dtype, ce_stream_t stream);
size_t ce_bag_backward_pradam_workspace(int64_t num_rows, int64_t nnz, int32_t dim, int32_t accumulator);
int ce_bag_backward_pradam(float* weight, int64_t num_rows, int32_t dim,
                           const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                           int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                           int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                           const uint64_t* presorted, const int32_t* row_of_slot, float* v, int64_t v_rows,
                           double beta1, double beta2, float lr, const float* lr_dev, float eps, float weight_decay,
                           int32_t weight_decay_mode, int64_t* step, int32_t accumulator, void* workspace,
                           size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_pradam_src(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                               const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                               const int32_t* row_of_slot, float* v, int64_t v_rows, double beta1, double beta2,
                               float lr, const float* lr_dev, float eps, float weight_decay, int32_t weight_decay_mode,
                               int64_t* step, int32_t accumulator, void* workspace, size_t workspace_bytes,
                               ce_stream_t stream);

/* Gradient clipping for the fused updates (additions to API 6): per value and per row norm.  Seven entries; each is an
 * existing argument list with `float grad_clip, int32_t grad_clip_mode` directly behind `weight_decay_mode`:
 *   ce_bag_backward_update_clip         the list of ce_bag_backward_update_wd
 *   ce_bag_backward_update_src_clip     the list of ce_bag_backward_update_src_wd
 *   ce_bag_backward_update_sorted_clip  the list of ce_bag_backward_update_sorted_wd
 *   ce_bag_backward_adam_clip           the list of ce_bag_backward_adam_wd
 *   ce_bag_backward_adam_src_clip       the list of ce_bag_backward_adam_src_wd
 *   ce_bag_backward_pradam_clip         the list of ce_bag_backward_pradam
 *   ce_bag_backward_pradam_src_clip     the list of ce_bag_backward_pradam_src
 * The workspaces and their zero-fill contract are those of the covered entries; so are the refusals, their codes,
 * messages and order, capture-safety, no host synchronisation, no allocation.
 *
 * g is the row's folded gradient of the call -- after per-sample weights, the mean scaling and the fold over the row's
 * lookups: what the covered entry's update starts from.  The clip acts on g FIRST, and everything that used g then uses
 * the clipped g: the L2 decay's h = g + wd * w, row-wise Adagrad's sum h^2 / dim, Adam's m' and v', partial row-wise
 * Adam's ss, the step -- the order of torch (clip_grad_* before optimizer.step()) and of FBGEMM (max_gradient).  fp32
 * with contraction off, every operation rounded on its own; c = grad_clip, a float by value:
 *   CE_CLIP_NONE      the covered entry's update, by the covered entry's kernels: its bits (grad_clip is not looked at)
 *   CE_CLIP_VALUE     per element:  g = g < -c ? -c : (g > c ? c : g)          (a NaN stays a NaN, as torch.clamp)
 *   CE_CLIP_ROW_NORM  ss = sum_d g[d]^2, per lane as row-wise Adagrad sums the squares for the table's type (an Adam
 *                     layout: the fp32 table's), then the xor tree across the row's lane group, widest stride first;
 *                     n = sqrtf(ss) ; k = c / (n + 1e-6f) ; if (k < 1.f) g[d] = g[d] * k    (clip_grad_norm_, every
 *                     row its own parameter)
 * Row-wise Adagrad and partial row-wise Adam then form their own sum of squares from the clipped (and decayed) gradient:
 * a second reduction, not k^2 * ss.  Clipping does not change which rows a call names: the mark rule depends on the
 * decay alone, a row with g = 0 stays a no-op for SGD and Adagrad without decay, and a slot whose momentum / v index
 * lies outside its array is still not touched.  A row looked up once in a call gets the same bits from CE_ACC_CACHE,
 * CE_ACC_STEP and the sorted entry.  grad_clip = +inf changes nothing (through the clipped kernels).
 * Refusals: an unknown grad_clip_mode, then -- with a mode other than CE_CLIP_NONE -- a grad_clip that is not > 0 (zero,
 * negative, NaN; +inf is taken) are CE_ERR_INVALID.  The two checks stand directly behind the weight-decay checks and
 * also apply for nnz == 0.  CE_OPT_SGD on an fp32 table stays CE_ERR_UNSUPPORTED in the two atomic entries (that scatter
 * has no per-row pass): fp32 SGD with clipping exists through the sorted entry only.
 * Not built: a global (whole-table) norm, FBGEMM's COUNTER / COWCLIP, a threshold read from device memory, clipping in
 * ce_rows_axpy. */
#define CE_CLIP_NONE 0
#define CE_CLIP_VALUE 1
#define CE_CLIP_ROW_NORM 2
int ce_bag_backward_update_clip(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                                int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                                int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                const uint64_t* presorted, const int32_t* row_of_slot, float* momentum,
                                int64_t momentum_rows, float lr, const float* lr_dev, float eps, float weight_decay,
                                int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode, int32_t optimizer,
                                int32_t rounding, uint64_t seed, int32_t accumulator, void* workspace,
                                size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_update_src_clip(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim, int64_t nnz,
                                    const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                    const int32_t* row_of_slot, float* momentum, int64_t momentum_rows, float lr,
                                    const float* lr_dev, float eps, float weight_decay, int32_t weight_decay_mode,
                                    float grad_clip, int32_t grad_clip_mode, int32_t optimizer, int32_t rounding,
                                    uint64_t seed, int32_t accumulator, void* workspace, size_t workspace_bytes,
                                    ce_stream_t stream);
int ce_bag_backward_update_sorted_clip(void* weight, int32_t weight_dtype, int64_t num_rows, int32_t dim,
                                       const int64_t* indices, int64_t nnz, const void* offsets,
                                       int32_t offsets_are_i64, int64_t num_bags, int32_t include_last_offset,
                                       const float* per_sample_weights, int32_t mode, int64_t hook_features,
                                       const void* grad_out, int32_t act_dtype, const int32_t* row_of_slot,
                                       float* momentum, int64_t momentum_rows, float lr, float eps, float weight_decay,
                                       int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode,
                                       int32_t optimizer, int32_t rounding, uint64_t seed, void* workspace,
                                       size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_adam_clip(float* weight, int64_t num_rows, int32_t dim,
                              const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                              int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                              int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                              const uint64_t* presorted, double beta1, double beta2, float lr, const float* lr_dev,
                              float eps, float weight_decay, int32_t weight_decay_mode, float grad_clip,
                              int32_t grad_clip_mode, int64_t* step, int32_t accumulator, void* workspace,
                              size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_adam_src_clip(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                  const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                  double beta1, double beta2, float lr, const float* lr_dev, float eps,
                                  float weight_decay, int32_t weight_decay_mode, float grad_clip,
                                  int32_t grad_clip_mode, int64_t* step, int32_t accumulator, void* workspace,
                                  size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_pradam_clip(float* weight, int64_t num_rows, int32_t dim,
                                const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                                int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                                int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                const uint64_t* presorted, const int32_t* row_of_slot, float* v, int64_t v_rows,
                                double beta1, double beta2, float lr, const float* lr_dev, float eps,
                                float weight_decay, int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode,
                                int64_t* step, int32_t accumulator, void* workspace, size_t workspace_bytes,
                                ce_stream_t stream);
int ce_bag_backward_pradam_src_clip(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                    const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                    const int32_t* row_of_slot, float* v, int64_t v_rows, double beta1, double beta2,
                                    float lr, const float* lr_dev, float eps, float weight_decay,
                                    int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode, int64_t* step,
                                    int32_t accumulator, void* workspace, size_t workspace_bytes, ce_stream_t stream);

/* Element-wise Adagrad with its state carried in the row, layout `adagrad` (additions to API 6; torch.optim.Adagrad,
 * FBGEMM's EXACT_ADAGRAD).  Row-wise Adagrad (ce_bag_backward_rowwise_adagrad*) keeps ONE sum of squares per row; this
 * is the optimizer it approximates, with one per element, and a state as large as the table travels in the row as
 * Adam's moments do.  An fp32 table only.  A row of `dim` elements is 2 * dim floats:
 *   w[0 .. dim) | h[dim .. 2 dim)                             (weights, sums of squared gradients)
 * The dim rule and the alignment are the Adam layout's (dim % 4 == 0, 4 <= dim <= 1024, the table 16-byte aligned;
 * vector lanes only; the cache op is driven with embedding_dim = 2 * dim).  `weight` is [num_rows, 2 * dim] in every
 * entry below; `dim` stays D.
 *
 * ce_host_fill_uniform_adagrad is ce_host_fill_uniform_pradam with every h element = init_acc (torch's
 * initial_accumulator_value) instead of zero: the same w parts, a result that does not depend on `threads`.
 * init_acc < 0 or NaN is CE_ERR_INVALID, before the dim rule (CE_ERR_UNSUPPORTED).
 *
 * ce_bag_forward_adagrad / ce_bag_forward_src_keys_adagrad take the lists of ce_bag_forward_pradam /
 * _src_keys_pradam and ARE those entries: a row two parts wide whose first part is read.  Bit-equal to the fp32
 * sibling's result over a contiguous copy of the w parts; the same refusals in the same order.
 *
 * ce_bag_backward_adagrad / ce_bag_backward_adagrad_src take the lists of ce_bag_backward_adam_clip / _adam_src_clip
 * with `double lr_decay` in place of `double beta1, double beta2`: decay and clip are in from the start.  lr / lr_dev,
 * `step`, the accumulators, the workspace (ce_bag_backward_adagrad_workspace = ce_bag_backward_adam_workspace) and its
 * zero-fill contract, the mark rule, capture safety, no host synchronisation and no allocation are the Adam entries'.
 * The arithmetic, fp32 with every operation rounded on its own (no contraction), for every UNIQUE row the call names, g
 * its folded gradient of the call, t the step count after the call's first launch added 1, lr the by-value rate or
 * *lr_dev as read when the kernels run:
 *     clr_d = (double)lr / (1.0 + (double)(t - 1) * lr_decay)                            fp64, on the device
 *     clr   = (float)clr_d
 *     g     = clip(g)                                                                    as in the _clip entries, first
 *     h  = g                                                                             no decay
 *     h  = g + weight_decay * w                                                          CE_WD_L2
 *     w  = w * f, h = g ; f = (float)(1.0 - clr_d * (double)weight_decay)                CE_WD_DECOUPLED
 *     s' = s + h * h                                                                     per element
 *     w' = w - clr * (h / (sqrtf(s') + eps))                                             per element
 *   With lr_decay == 0, clr == lr and f is the _wd entries' factor.  A replayed graph follows *lr_dev and *step in both
 *   clr and f.
 *   - Rows no covered lookup names keep w and s bit for bit.  Lookups outside [0, num_rows) and lookups no bag covers
 *     take no part and flag nothing.  A row named only by zero-weight lookups has g = 0: without decay s + 0 and w - 0
 *     leave its bits as they were.  eps == 0 on a zero state gives NaN (0 / 0), as in torch.  Given the same folded
 *     gradient both accumulators write the same bits: no reduction across lanes outside the row-norm clip.
 *   - Refused before the first launch, in the Adam entries' order: step == NULL first; then the accumulator code, the
 *     decay's and the clip's checks; lr_decay < 0 or NaN, eps < 0, lr < 0 (CE_ERR_INVALID); act_dtype; the dim rule
 *     (CE_ERR_UNSUPPORTED); null pointers, sizes, alignment, workspace.  nnz == 0 (or num_bags == 0) returns after the
 *     checks with no launch: it does not count a step.
 * Not built: 16-bit state or tables, a scalar lane form.  (The sorted fold: ce_bag_backward_adagrad_sorted.) */
int ce_host_fill_uniform_adagrad(float* dst, int64_t n_rows, int32_t dim, float lo, float hi, uint64_t seed,
                                 float init_acc, int threads);
int ce_bag_forward_adagrad(const float* weight, int64_t num_rows, int32_t dim,
                           const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                           int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                           int32_t mode, int64_t hook_features, void* out, int32_t act_dtype, ce_stream_t stream);
int ce_bag_forward_src_keys_adagrad(const float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                    const uint64_t* src_keys, void* out, int32_t act_dtype, ce_stream_t stream);
size_t ce_bag_backward_adagrad_workspace(int64_t num_rows, int64_t nnz, int32_t dim, int32_t accumulator);
int ce_bag_backward_adagrad(float* weight, int64_t num_rows, int32_t dim,
                            const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                            int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                            int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                            const uint64_t* presorted, double lr_decay, float lr, const float* lr_dev, float eps,
                            float weight_decay, int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode,
                            int64_t* step, int32_t accumulator, void* workspace, size_t workspace_bytes,
                            ce_stream_t stream);
int ce_bag_backward_adagrad_src(float* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                                const void* grad_out, int32_t act_dtype, const uint64_t* src_keys,
                                double lr_decay, float lr, const float* lr_dev, float eps, float weight_decay,
                                int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode, int64_t* step,
                                int32_t accumulator, void* workspace, size_t workspace_bytes, ce_stream_t stream);

/* Deterministic, accumulator-free updates of the three in-row layouts (additions to API 6): what
 * ce_bag_backward_update_sorted is to SGD and row-wise Adagrad, for the Adam layout (rows w | m | v), partial row-wise
 * Adam (rows w | m, v per table row) and element-wise Adagrad (rows w | h).  Bit-reproducible, no atomics, a workspace
 * proportional to the call's lookups.
 *   ce_bag_backward_adam_sorted     the list of ce_bag_backward_adam_clip   without `presorted` and `accumulator`
 *   ce_bag_backward_pradam_sorted   the list of ce_bag_backward_pradam_clip without `presorted` and `accumulator`
 *   ce_bag_backward_adagrad_sorted  the list of ce_bag_backward_adagrad     without `presorted` and `accumulator`
 * Decay and clip are always in the list; weight_decay 0 / CE_WD_NONE and CE_CLIP_NONE select the kernels without them.
 *   - The fold is ce_bag_backward_update_sorted's, CE_SORTED_CHUNK = 64: the lookups stably sorted by slot; a run of
 *     n <= 64 lookups folded strictly in lookup order in fp32 from zero, g = (...((s_0 g_0) + s_1 g_1) + ...), the term
 *     the gradient row itself for s_j == 1 and otherwise the product rounded before it is added; s_j the per-sample
 *     weight, 1 / len for mean (both together: their quotient); a 16-bit grad_out upcast exactly; a longer run cut into
 *     chunks of 64 positions counted from the start of the run, each folded from zero, the partial rows added in
 *     ascending chunk order.  Nothing depends on the grid, on the slot a row sits in or on timing.
 *   - Which rows: the atomic in-row entries' rule.  A row is updated once per call iff a lookup that a bag covers names
 *     it, zero weights or not (such a row decays, its moments decay towards zero).  Lookups outside [0, num_rows) and
 *     lookups no bag covers head nothing; a row only they name keeps every part bit for bit.  Partial row-wise Adam: a
 *     slot whose row_of_slot lies outside [0, v_rows) is left alone.
 *   - The update of a row from its folded gradient is the atomic entries' -- clip, decay, moments or sums of squares, w
 *     -- by the same device function: given the same folded gradient a row gets the bits of CE_ACC_CACHE / CE_ACC_STEP.
 *   - The call's first launch adds 1 to *step; the step size, the decayed Adagrad rate and the decoupled factor are
 *     formed on the device from lr or *lr_dev and *step, so a captured call that is replayed follows the count and a
 *     schedule.  One stream, no host synchronisation, no allocation, launch shapes fixed by the arguments; nothing in
 *     the workspace needs initialising, and no state passes from call to call except the table, v and *step.
 *   - ce_bag_backward_in_row_sorted_workspace(num_rows, nnz, dim): 256-byte aligned, independent of num_rows; the sort's
 *     arrays and one partial row of dim floats per lookup (0 for nnz < 0, nnz >= 2^31 - 1 or dim <= 0).
 *   - Refused before the first launch and before any HIP call, the table untouched, in this order: step == NULL; the
 *     decay's checks; the clip's checks; betas outside [0, 1), or lr_decay < 0 or NaN; eps < 0; lr < 0 (by value only);
 *     act_dtype; null pointers (weight, grad_out, workspace; v for partial row-wise Adam); sizes (dim <= 0, num_rows,
 *     nnz, num_bags); mode other than sum / mean (CE_ERR_UNSUPPORTED); hook_features; alignment (table 16 bytes, step 8,
 *     grad_out on its vector boundary, workspace 256) and the workspace's size; the dim rule, dim % 4 == 0 and
 *     4 <= dim <= 1024 (CE_ERR_UNSUPPORTED).  nnz == 0 or num_bags == 0 then returns with no launch and counts no step;
 *     otherwise indices == NULL or offsets == NULL is CE_ERR_INVALID.
 * Not built: a form from source-row keys, 16-bit tables or moments, stochastic rounding, mode max, scalar lanes. */
size_t ce_bag_backward_in_row_sorted_workspace(int64_t num_rows, int64_t nnz, int32_t dim);
int ce_bag_backward_adam_sorted(float* weight, int64_t num_rows, int32_t dim,
                                const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                                int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                                int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                double beta1, double beta2, float lr, const float* lr_dev, float eps,
                                float weight_decay, int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode,
                                int64_t* step, void* workspace, size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_pradam_sorted(float* weight, int64_t num_rows, int32_t dim,
                                  const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                                  int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                                  int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                  const int32_t* row_of_slot, float* v, int64_t v_rows, double beta1, double beta2,
                                  float lr, const float* lr_dev, float eps, float weight_decay,
                                  int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode, int64_t* step,
                                  void* workspace, size_t workspace_bytes, ce_stream_t stream);
int ce_bag_backward_adagrad_sorted(float* weight, int64_t num_rows, int32_t dim,
                                   const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                                   int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                                   int32_t mode, int64_t hook_features, const void* grad_out, int32_t act_dtype,
                                   double lr_decay, float lr, const float* lr_dev, float eps, float weight_decay,
                                   int32_t weight_decay_mode, float grad_clip, int32_t grad_clip_mode, int64_t* step,
                                   void* workspace, size_t workspace_bytes, ce_stream_t stream);

/* 8-bit row-wise quantized table, `q8` (additions to API 6): evaluation and serving only -- there is NO backward and
 * no update; a q8 table is built from trained rows (ce_host_quantize_q8) and written only by
 * ce_cache_install_rows.
 * A row of `dim` elements is 16 + dim bytes:
 *   bytes 0..3 scale (fp32) | 4..7 bias (fp32) | 8..15 zero | 16..16+dim-1: dim codes, uint8
 * dim % 16 == 0, 16 <= dim <= 1024 and the table 16-byte aligned, so every row is a whole number of 16-byte units
 * and its codes start 16-byte aligned (the cache op, which only moves rows, is driven with embedding_dim =
 * (16 + dim) / 4).  Any other dim: CE_ERR_UNSUPPORTED before any launch; ce_q8_row_bytes returns 0 for it.
 * Element value: v = fmaf((float)q, scale, bias) -- ONE explicit fused multiply-add, in the kernels and on the host.
 * Quantizer (fp32 IEEE throughout, every operation rounded to fp32, no contraction), per row: lo = min, hi = max,
 * scale = (hi - lo) / 255, bias = lo, q = clamp(rintf((x - lo) / scale), 0, 255) (ties to even).  If the fp32
 * quotient (hi - lo) / 255 is 0 (a constant row, a denormal range) all codes are 0 and scale is stored as 0: the row
 * reproduces lo.  A row holding a NaN or an infinity: CE_ERR_INVALID, ce_last_error names the first such row, and
 * the destination is unspecified.  The result does not depend on `threads` (capped by ce_cpu_budget()).
 * src_dtype: CE_ACT_F32 / CE_ACT_BF16 / CE_ACT_F16 (16-bit sources are up-converted exactly first).  Both host
 * entries work on host memory and need no GPU.
 * The two forwards are ce_bag_forward_w16 / ce_bag_forward_src_keys_w16 in every respect but the row type: sum /
 * mean, per-sample weights, hook_features, int32 / int64 offsets, offsets == NULL for one id per bag; lookups outside
 * [0, num_rows) take no part (the key-driven form writes a zero row for them); fp32 sums, one rounding on the store
 * to act_dtype; capture-safe; everything refusable is refused before the first launch. */
#define CE_Q8_HEADER_BYTES 16
size_t ce_q8_row_bytes(int32_t dim);
int ce_host_quantize_q8(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, void* dst, int threads);
int ce_host_dequantize_q8(const void* src, int64_t n_rows, int32_t dim, float* dst, int threads);
int ce_bag_forward_q8(const void* weight, int64_t num_rows, int32_t dim,
                      const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                      int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                      int32_t mode, int64_t hook_features, void* out, int32_t act_dtype, ce_stream_t stream);
int ce_bag_forward_src_keys_q8(const void* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                               const uint64_t* src_keys, void* out, int32_t act_dtype, ce_stream_t stream);

/* 4-bit row-wise quantized table, `q4` (additions to API 6): q8 with 16 levels -- evaluation and serving only, no
 * backward, no update, written only by ce_cache_install_rows.  A row of `dim` elements is 16 + dim / 2 bytes:
 *   bytes 0..3 scale (fp32) | 4..7 bias (fp32) | 8..15 zero | 16..16+dim/2-1: dim codes, two per byte
 * Element i is in code byte i / 2: the low nibble for even i, the high nibble for odd i.  The four elements
 * 4ch .. 4ch+3 of a lane's chunk ch are therefore one little-endian uint16 at code offset 2ch, nibble k of it is
 * element 4ch + k.
 * dim % 32 == 0, 32 <= dim <= 1024 and the table 16-byte aligned, so every row is a whole number of 16-byte units and
 * its codes start 16-byte aligned (the cache op is driven with embedding_dim = (16 + dim / 2) / 4).  Any other dim:
 * CE_ERR_UNSUPPORTED before any launch; ce_q4_row_bytes returns 0 for it.
 * The header is q8's 16 bytes (fp32 scale and bias, 8 zero bytes) for the same alignment reason: the fp16 scale / bias
 * that FBGEMM's 4-bit rows carry BEHIND the codes is not followed, and such rows are not read.
 * Element value: v = fmaf((float)q, scale, bias) -- ONE explicit fused multiply-add, in the kernels and on the host.
 * Quantizer: q8's with 15 in place of 255 -- scale = (hi - lo) / 15, bias = lo, q = clamp(rintf((x - lo) / scale), 0,
 * 15); a zero quotient stores scale 0 and codes 0; a NaN or an infinity is CE_ERR_INVALID naming the first such row;
 * the result does not depend on `threads`; both nibbles of every code byte and the pad bytes are written.
 * Every entry has the argument list of its q8 twin and behaves like it in every respect but the row type. */
#define CE_Q4_HEADER_BYTES 16
size_t ce_q4_row_bytes(int32_t dim);
int ce_host_quantize_q4(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, void* dst, int threads);
int ce_host_dequantize_q4(const void* src, int64_t n_rows, int32_t dim, float* dst, int threads);
int ce_bag_forward_q4(const void* weight, int64_t num_rows, int32_t dim,
                      const int64_t* indices, int64_t nnz, const void* offsets, int32_t offsets_are_i64,
                      int64_t num_bags, int32_t include_last_offset, const float* per_sample_weights,
                      int32_t mode, int64_t hook_features, void* out, int32_t act_dtype, ce_stream_t stream);
int ce_bag_forward_src_keys_q4(const void* weight, int64_t num_rows, int32_t dim, int64_t nnz,
                               const uint64_t* src_keys, void* out, int32_t act_dtype, ce_stream_t stream);

/* Device-side quantizer (additions to API 6): the rows ce_host_quantize_q8 / _q4 write, byte for byte -- scale, bias,
 * the 8 zero bytes and the codes (both nibbles of every q4 byte) --, from rows that are in device memory already.
 * src: [n_rows, dim] fp32, bf16 or fp16 (src_dtype: CE_ACT_*), device memory, 16-byte aligned (8 for a 16-bit source);
 * dst: [n_rows, ce_q8_row_bytes(dim)] (ce_q4_row_bytes(dim)), device memory, 16-byte aligned.  first_bad: one device
 * int64 -- the entry sets it to INT64_MAX on `stream`, the kernel lowers it (an ordinary global atomic minimum) to the
 * smallest index of a row that holds a NaN or an infinity or whose range overflows fp32; such a row's destination is
 * unspecified, every other row is written.  Asynchronous on `stream`; the entry does not read first_bad back.
 * Refused before any launch, as the host entries refuse it: an unknown src_dtype, a negative n_rows, a null pointer, a
 * misaligned one (CE_ERR_INVALID), the dim rule (CE_ERR_UNSUPPORTED); n_rows == 0 is CE_OK.
 * The arithmetic is the quantizer's above, operation by operation: bias is the FIRST element equal to the minimum, in
 * index order (the sign of a zero minimum follows it); both divisions are correctly rounded fp32, subnormal operands
 * and quotients included; rintf rounds the ties to even. */
int ce_quantize_rows_q8(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, void* dst, int64_t* first_bad,
                        ce_stream_t stream);
int ce_quantize_rows_q4(const void* src, int32_t src_dtype, int64_t n_rows, int32_t dim, void* dst, int64_t* first_bad,
                        ce_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * CachedParamMgr [A.1-A.6]. Device state arrays are owned by the caller (so the Python
 * mirror can expose them as tensors: cached_idx_map, inverted_cached_idx, idx_map,
 * freq_cnter, cuda_cached_weight); the library owns only the opaque scratch it is handed.
 * Row ids are int32 on the device (num_embeddings < 2^31), counters int64.
 */
typedef struct ce_cache_config {
  int64_t num_embeddings;        /* N: rows of the host table                              */
  int64_t cuda_row_num;          /* C: rows resident in HBM (int(N*cache_ratio), A.7)       */
  int32_t embedding_dim;         /* D (fp32 elements per row)                              */
  int32_t evict_strategy;        /* CE_EVICT_*                                             */
  int32_t transport;             /* CE_TRANSPORT_*                                         */
  int32_t protect_depth;         /* 0 = reference semantics; d>0 also protects the rows of
                                    the previous d prepare_ids calls (overlapped pipeline)  */
  int64_t max_ids_per_call;      /* upper bound of n in ce_cache_prepare_ids                */
  float* host_weight;            /* [N, D] host table, HOST address                        */
  float* host_weight_dev;        /* same memory, DEVICE-visible address (ce_host_*)        */
  float* cache_weight;           /* device [C, D]  cuda_cached_weight                      */
  int32_t* idx_map;              /* device int32[N] id -> cpu_row_idx, NULL = identity     */
  int32_t* inverted_cached_idx;  /* device int32[N] cpu_row_idx -> slot, -1 = absent (16-B aligned) */
  int32_t* cached_idx_map;       /* device int32[C] slot -> cpu_row_idx, -1 = empty        */
  int64_t* freq_cnter;           /* device int64[C] (LFU) or NULL; ignored under LRU       */
  void* workspace;               /* device scratch, ce_cache_workspace_bytes() bytes       */
  size_t workspace_bytes;
} ce_cache_config_t;

/* per-call statistics [A.3-4]: what num_hits_history / num_miss_history /
 * num_write_back_history record (recsys/dlrm_main.py:286-289) */
typedef struct ce_call_stats {
  int64_t seq;          /* call number, 1-based                      */
  int64_t n_ids;        /* ids in the call                           */
  int64_t n_unique;     /* unique rows                               */
  int64_t n_miss;       /* unique rows not resident                  */
  int64_t n_evict;      /* rows written back + evicted               */
  int64_t miss_lookups; /* sum of multiplicities of missed rows      */
  int64_t n_free_after; /* free slots after the call                 */
  int32_t status;       /* CE_OK, CE_ERR_CAPACITY or CE_ERR_RANGE    */
  int32_t kind;         /* CE_CALL_*                                 */
} ce_call_stats_t;

#define CE_CALL_PREPARE 0
#define CE_CALL_PRELOAD 1
#define CE_CALL_FLUSH 2

size_t ce_cache_workspace_bytes(int64_t num_embeddings, int64_t cuda_row_num, int64_t max_ids_per_call,
                                int32_t embedding_dim);

/* Builds the manager over caller-owned arrays and initialises them to the empty-cache
 * state of A.1 (maps = -1, freq_cnter = INT64_MAX, cache rows untouched).  Blocks. */
int ce_cache_create(const ce_cache_config_t* cfg, ce_stream_t stream, ce_cache_t** out);
int ce_cache_destroy(ce_cache_t* h);

/* Warm-up preload of reorder() [A.2-2]: rows[i] (device int32, NULL = i) -> slot i for
 * i < n, with freq_vals (device int64, NULL = 0) written to freq_cnter under LFU. */
int ce_cache_preload(ce_cache_t* h, const int32_t* rows, const int64_t* freq_vals, int64_t n,
                     ce_stream_t stream);

/* LFU only: tells the manager that no freq_cnter value exceeds `bound` (the largest value handed to
 * ce_cache_preload); together with the ids seen since, this bounds every counter and lets the victim select skip the
 * radix passes above it.  Optional: without it the select runs all 8 byte passes until the bound is known.
 * Under the other strategies it does nothing and returns CE_OK. */
int ce_cache_set_freq_bound(ce_cache_t* h, int64_t bound);

/* prepare_ids [A.3] -- recsys/dlrm_main.py:259: unique rows of `ids` (device int64[n]; any id outside
 * [0, num_embeddings) -- -1 included -- fails the call with CE_ERR_RANGE, as upstream's idx_map.index_select raises) are
 * made resident (victim selection A.5 with the canonical tie rule, write-back, admit A.4),
 * slots_out (device int64[n]) receives inverted_cached_idx[idx_map[ids]] [A.6], LFU
 * counters gain the multiplicities.  Fully asynchronous on `stream`.  On overflow or a bad
 * id the call leaves every piece of state untouched and flags the status in its stats.
 * slots_out is SCRATCH from the call's first kernel on (the row of every id is parked there and converted to its slot
 * in place by the last kernel): nothing may read or write it on another stream until the call has finished, and it
 * must not alias `ids`. */
int ce_cache_prepare_ids(ce_cache_t* h, const int64_t* ids, int64_t n, int64_t* slots_out,
                         ce_stream_t stream);
/* prepare_ids for a prefetch window of n_batches equal batches (ids = [n_batches, nnz_per_batch]) that also leaves
 * the window's keys in keys_out (device uint64[n_batches * ce_bag_presort_len(nnz_per_batch)]): what
 * ce_cache_prepare_ids followed by ce_bag_presort_window (src_keys == 0) or ce_bag_presort_window_src (src_keys != 0;
 * the offsets / num_bags / include_last_offset / hook_features arguments as there) produce, but the call's last kernel
 * converts the rows to slots AND writes the keys in ONE pass instead of writing 8 bytes of slot per id for the presort
 * to read straight back (the reference's `_train` window block, recsys/dlrm_main.py:243-262, plus this build's
 * window presort).  slots_out is still filled.  Capturable like ce_cache_prepare_ids. */
int ce_cache_prepare_ids_keys(ce_cache_t* h, const int64_t* ids, int64_t n_batches, int64_t nnz_per_batch,
                              int64_t* slots_out, int32_t src_keys, const void* offsets, int32_t offsets_are_i64,
                              int64_t offsets_batch_stride, int64_t num_bags, int32_t include_last_offset,
                              int64_t hook_features, uint64_t* keys_out, ce_stream_t stream);
/* ce_cache_prepare_ids_keys (keys_out != NULL) or ce_cache_prepare_ids over a [n_batches, nnz_per_batch] window
 * (keys_out == NULL) issued in TWO HALVES on one stream, so that a caller can put work of its own between them:
 *   _begin   unique rows, misses (the admission worker starts fetching them); with the zero-copy / staged transports
 *            also victim selection, staging of the victims and the free-slot list -- everything that needs nothing from
 *            the host table;
 *   _finish  (worker transport, API 5: victim selection, staging of the victims -- the write-back worker takes them --,
 *            free-slot list: beside the admission kernel's PCIe reads these kernels ran 2-3 x slower than alone, behind
 *            the caller's steps they run alone and the admission starts as early as before; CE_SPLIT_AFTER_EMIT=0
 *            restores the API-4 split point), then the wait for the admitted rows, their unpacking, the map updates,
 *            slots (and keys).
 * Why: run on a side stream beside the training kernels, the cache op's kernels and the bag kernels slow each other
 * down by MORE than the cache op's own kernel time (all of them are bound by the same memory system); issued on the
 * TRAINING stream as begin(window k+1) -> the steps of window k -> finish(window k+1), nothing runs beside anything,
 * and the one thing that does take wall time without using the GPU -- the PCIe admission -- still overlaps with the
 * steps in between.  Window k's rows must be protected while the cache op of window k+1 selects victims:
 * protect_depth >= 1.
 * No other call on the handle between the two; not capturable. */
int ce_cache_prepare_ids_begin(ce_cache_t* h, const int64_t* ids, int64_t n_batches, int64_t nnz_per_batch,
                               int64_t* slots_out, int32_t src_keys, const void* offsets, int32_t offsets_are_i64,
                               int64_t offsets_batch_stride, int64_t num_bags, int32_t include_last_offset,
                               int64_t hook_features, uint64_t* keys_out, ce_stream_t stream);
int ce_cache_prepare_ids_finish(ce_cache_t* h, ce_stream_t stream);
/* The same, for callers whose id lists are PADDED to a fixed capacity (the row-wise exchange's fixed-size buckets):
 * an entry of -1 is padding -- it takes no part in the call and gets slot -1.  Every other id outside the table still
 * fails the call.  Opt-in on purpose: on the plain entry point a -1 sentinel leaking out of a data pipeline must fail
 * loudly, not train on zero rows. */
int ce_cache_prepare_ids_padded(ce_cache_t* h, const int64_t* ids, int64_t n, int64_t* slots_out,
                                ce_stream_t stream);
/* First half of ce_cache_prepare_ids_padded (API 5): as ce_cache_prepare_ids_begin, for a padded id list and without
 * keys; ce_cache_prepare_ids_finish enqueues the second half.  The owner-side cache op of the row-wise exchange in its
 * one-stream arrangement (parallel.GraphedShardedWindow(arrangement="interleaved")). */
int ce_cache_prepare_ids_begin_padded(ce_cache_t* h, const int64_t* ids, int64_t n, int64_t* slots_out,
                                      ce_stream_t stream);

/* Worker transport, chained admission (API 6; the default when the host table has a device mapping): the missed rows
 * of a call travel on a private admission stream -- admission kernel behind the call's front, unpack kernel behind its
 * victim selection -- while the call's own stream goes on with selection, maps and slots.  By default a prepare_ids
 * call (or its _finish half) ENDS by making its stream wait for the rows, so "everything the call did is ordered
 * before whatever the caller enqueues next on that stream" holds as for every other transport.
 * A pipeline that issues the next cache op on the same stream before anything reads the cache (prefetch_num = 1 with
 * the cache op on a side stream) can take that wait out of the cache-op stream's chain:
 *   ce_cache_set_deferred_rows(h, 1)   calls no longer wait for their rows;
 *   ce_cache_rows_ticket(h)            ticket of the most recent call (0: no chained call yet);
 *   ce_cache_wait_rows(h, t, stream)   `stream` waits until the rows of call `t` (and of every call before it) are in
 *                                      their slots -- before the first kernel that reads the cache rows of that call's
 *                                      slots.  t <= 0: the most recent call.  A no-op for the other transports.
 * ce_cache_flush / _preload / _last_stats / _set_transport order themselves behind the rows whatever the setting. */
int ce_cache_set_deferred_rows(ce_cache_t* h, int32_t on);
int64_t ce_cache_rows_ticket(ce_cache_t* h);
int ce_cache_wait_rows(ce_cache_t* h, int64_t ticket, ce_stream_t stream);

/* Blocks until the most recent prepare_ids/preload/flush has finished on the device and
 * returns that call's statistics; returns its status (CE_ERR_CAPACITY ...). */
int ce_cache_last_stats(ce_cache_t* h, ce_call_stats_t* out);
/* Non-blocking totals accumulated from finished calls (call ce_cache_last_stats first for
 * exact values): _cpu_to_cuda_numel, _cuda_to_cpu_numel, _cache_miss, _total_cache. */
int ce_cache_totals(ce_cache_t* h, int64_t* cpu_to_cuda_numel, int64_t* cuda_to_cpu_numel,
                    int64_t* cache_miss, int64_t* total_cache, int64_t* n_calls);
/* Non-blocking: how many FINISHED calls ended with a status other than CE_OK (capacity overflow, bad id), and the
 * status / call number of the latest one.  A pipeline that never blocks on a call's record (strict = False) polls
 * this once per window and raises the reference's AssertionError one window late instead of never. */
int ce_cache_failures(ce_cache_t* h, int64_t* n_failed, int32_t* last_status, int64_t* last_seq);
/* Copies up to `cap` per-call records of finished calls starting at call `first_seq` (the library keeps the most
 * recent 65536 records). */
int64_t ce_cache_history(ce_cache_t* h, int64_t first_seq, ce_call_stats_t* out, int64_t cap);

/* _id_to_cached_cuda_id [A.6] alone (no cache maintenance): slots_out = inverted[idx_map[ids]] */
int ce_cache_lookup_slots(ce_cache_t* h, const int64_t* ids, int64_t n, int64_t* slots_out,
                          ce_stream_t stream);

/* flush() [A.7]: every resident row is written back to the host table, maps emptied,
 * freq_cnter reset.  Asynchronous on `stream`. */
int ce_cache_flush(ce_cache_t* h, ce_stream_t stream);

/* Refresh rows in place, behind the cache (addition to API 6): rows[i] -- 4 * embedding_dim bytes in the TABLE's row
 * format, which this entry never interprets (fp32, 16-bit, q8 and q4 tables alike) -- becomes the value of row
 * idx_map[ids[i]] in EVERY live copy: the host row (through the table's device mapping) and, where the row is
 * resident, its cache slot.  ids (id space) and rows are device memory; rows keeps the table's alignment.  ids must be
 * distinct: with duplicates a row's copies are unspecified.
 * It opens the way ce_cache_flush opens: a call begun with ce_cache_prepare_ids_begin is CE_ERR_INVALID; with the
 * worker transport every queued write-back lands first (one still on its way may carry an old copy of a row being
 * installed); `stream` waits for the rows of the chained admission.  Behind it the previous write-back job's staging
 * buffer is no longer probed by the next admission (it may hold the old payload of a row evicted by the last call).
 * An id outside [0, num_embeddings): CE_ERR_RANGE, nothing is written.  Admits nothing, evicts nothing, and touches no
 * map, counter, stamp, statistic or history record.  SYNCHRONOUS: it returns after its kernels have finished, so the
 * host table can be read straight away.  Refused inside a stream capture (CE_ERR_UNSUPPORTED). */
int ce_cache_install_rows(ce_cache_t* h, const int64_t* ids, int64_t n, const void* rows, ce_stream_t stream);

int ce_cache_set_protect_depth(ce_cache_t* h, int32_t depth);
/* Switching away from / to CE_TRANSPORT_WORKER blocks until the queued write-backs have landed. */
int ce_cache_set_transport(ce_cache_t* h, int32_t transport);
/* The transport in force (CE_TRANSPORT_*).  It can differ from what was set: the first prepare_ids on a stream runs a
 * self-test of the worker transport (do the library's copy streams make progress while that stream is parked in
 * hipStreamWaitValue64? -- a property of the process's HIP runtime settings, e.g. GPU_MAX_HW_QUEUES) and falls back
 * to CE_TRANSPORT_ZEROCOPY, with a message on stderr, when they do not. */
int32_t ce_cache_get_transport(ce_cache_t* h);
/* Move the cache to another allocation (API 3): `cache_weight` = device fp32 [>= cuda_row_num, D] whose first
 * cuda_row_num rows the caller has filled with the current cache contents.  Blocks until the device is idle, then
 * every later call addresses the new rows.  Lets a caller keep extra rows right BEHIND the cache in one allocation
 * (the row-wise exchange's receive buffer: ce_exchange_local_index).  No upstream counterpart: upstream's
 * cuda_cached_weight is a torch tensor the caller owns (cache_mgr.py:83-89). */
int ce_cache_set_cache_weight(ce_cache_t* h, float* cache_weight);
/* A cache op inside the caller's hipGraph (API 3).  ce_cache_prepare_ids issued while `stream` is being captured
 * (hipStreamBeginCapture) records its kernels into that capture instead of running them: zero-copy transport only,
 * phase timers off; ids / slots_out must stay valid for every replay.  The call number that dates the eviction
 * backlist and addresses the stats ring is then counted on the device, and the caller reports the replays --
 * n_calls captured calls of ids_per_call ids each, just launched on `stream` -- right after every hipGraphLaunch:
 * this keeps the host's call count, the stats history and (LFU) the counter bound in step.  CE_ERR_UNSUPPORTED from it
 * means an LFU capture has outlived the key width it was captured with (2^31 ids): capture again.  With it the
 * whole step of a prefetch_num = 1 loop -- cache op of batch k+1 beside forward + backward of batch k -- is ONE graph
 * launch instead of ~16 kernel launches (recsys/dlrm_main.py:256-279 is the loop this replaces). */
int ce_cache_graph_replayed(ce_cache_t* h, int64_t n_calls, int64_t ids_per_call, ce_stream_t stream);
/* Phase timers of prepare_ids (upstream's per-phase Timer / record_function ranges, recsys/dlrm_main.py:258,294):
 * when on, every call brackets its phases with hipEvents on its own stream (no host sync); ce_cache_phase_times
 * blocks until the calls issued so far have finished and returns the accumulated milliseconds per phase
 * (ce_cache_phase_count() values, named by ce_cache_phase_name) and the number of calls they cover. */
int ce_cache_set_profiling(ce_cache_t* h, int32_t on);
int32_t ce_cache_phase_count(void);
const char* ce_cache_phase_name(int32_t i);
int ce_cache_phase_times(ce_cache_t* h, double* ms_out, int32_t cap, int64_t* calls, int32_t reset);
/* CE_TRANSPORT_WORKER: blocks until every eviction of the calls issued so far has reached the host table (the
 * reference's `weight` is current the moment prepare_ids returns; with the worker transport it is current after
 * this call or after ce_cache_flush).  No-op for the other transports. */
int ce_cache_writeback_wait(ce_cache_t* h);
/* Worker-side accounting of the row swap (upstream's swap_out_bandwidth / swap_in_bandwidth, printed by
 * print_comm_stats, recsys/dlrm_main.py:294): seconds6 = {out: waiting for staging, out: copying + scattering,
 * in: waiting for the miss list and earlier write-backs, in: gathering + copying, in: of which gathering +
 * enqueueing the copies, (a count, not seconds) admission jobs that ran while the previous call's write-back was
 * still on its way -- the rows that call evicted were taken from its staging buffer in HBM}, counts4 = {rows out,
 * jobs out, rows in, jobs in}. */
int ce_cache_swap_stats(ce_cache_t* h, double* seconds6, int64_t* counts4);
/* upstream buffer_size / LimitBuffIndexCopyer: rows > 0 bounds the pinned + device staging of the STAGED
 * transport to `rows` rows; larger swaps walk it in chunks.  0 (default) = stage a whole swap at once. */
int ce_cache_set_buffer_rows(ce_cache_t* h, int64_t rows);
/* number of free slots as of the last finished call (blocks like ce_cache_last_stats) */
int ce_cache_free_rows(ce_cache_t* h, int64_t* out);

/* ---------------------------------------------------------------------------------------
 * Row-wise sharding helpers (BASELINE.json north_star): the build's
 * replacement for KJTAllToAll (recsys/datasets/utils.py:20-54).  Rows are owned by
 * rank = row % world, local row = row / world.
 * ce_bucketize_rows: ids (device int64[n]) -> rows via idx_map (NULL = identity), stable
 * counting sort by owner: local_rows_out[perm position] = row / world (int64),
 * perm_out[j] = position of lookup j in the bucketed order, counts_out[w] (device int64[world]).
 */
size_t ce_bucketize_workspace(int64_t n, int32_t world);
int ce_bucketize_rows(const int64_t* ids, int64_t n, const int32_t* idx_map, int32_t world,
                      int64_t* local_rows_out, int64_t* perm_out, int64_t* counts_out,
                      void* workspace, size_t workspace_bytes, ce_stream_t stream);

/* ce_dedupe_bucket_rows: what the row-wise exchange uses instead of ce_dedupe_rows + ce_bucketize_rows: the
 * batch's unique rows, grouped by owner (row % world, any order inside a bucket), as local rows
 * (row / world) in local_rows_out[0 .. sum(counts)), pos_out[j] = position of lookup j's row in that list
 * (-1 for an id outside [0, num_rows)), counts_out[w] = unique rows owned by w (device int64[world]).
 * stamp, slot_of_row: device int32[num_rows] scratch owned by the caller (no initialisation needed, contents
 * are meaningless between calls); slot_of_row may be NULL: the stamp array then serves both purposes (4 bytes of
 * scratch per table row instead of 8 -- per batch of a window in the _window form); scratch: device
 * int32[(world + 1) * n].  world <= 64.
 * No host sync: the bucket sizes stay on the device (the caller all-to-alls them as a fixed-size message). */
int ce_dedupe_bucket_rows(const int64_t* ids, int64_t n, const int32_t* idx_map, int64_t num_rows,
                          int32_t world, int32_t* stamp, int32_t* slot_of_row, int32_t* scratch,
                          int64_t* local_rows_out, int64_t* pos_out, int64_t* counts_out, ce_stream_t stream);

/* Fixed-capacity form (API 3) for the graphed exchange: bucket w occupies local_rows_out[w * capacity, (w + 1) *
 * capacity) (device int64[world * capacity], unused places = -1) and pos_out[j] = w * capacity + place, so nothing a
 * training step touches has a data-dependent size and a window's steps -- padded, equal-split all-to-alls included --
 * replay as one hipGraph.  A bucket larger than `capacity` sets *overflow_flag (device int32, caller-zeroed) and its
 * surplus lookups get pos -1: the caller re-plans that window on the variable-size path.  Padding rows (-1) are
 * accepted by ce_cache_prepare_ids as "no lookup" (slot -1). */
int ce_dedupe_bucket_rows_padded(const int64_t* ids, int64_t n, const int32_t* idx_map, int64_t num_rows,
                                 int32_t world, int64_t capacity, int32_t* stamp, int32_t* slot_of_row,
                                 int32_t* scratch, int64_t* local_rows_out, int64_t* pos_out, int64_t* counts_out,
                                 int32_t* overflow_flag, ce_stream_t stream);

/* The same for the n_batches batches of a window in one launch per pass (3 launches instead of 3 per batch): ids =
 * device int64 [n_batches, n] contiguous, outputs [n_batches, world * capacity] / [n_batches, n] / [n_batches, world];
 * stamp and slot_of_row = device int32 [n_batches * num_rows] EACH (one array per batch: concurrent batches would race
 * on a row's entry), scratch = device int32 [n_batches * (world + 1) * n]; one overflow flag for the window. */
int ce_dedupe_bucket_rows_padded_window(const int64_t* ids, int64_t n, int64_t n_batches, const int32_t* idx_map,
                                        int64_t num_rows, int32_t world, int64_t capacity, int32_t* stamp,
                                        int32_t* slot_of_row, int32_t* scratch, int64_t* local_rows_out,
                                        int64_t* pos_out, int64_t* counts_out, int32_t* overflow_flag,
                                        ce_stream_t stream);

/* Local bypass of the row-wise exchange (API 3).  pos: device int64 [n_batches, n_per_batch], the places
 * ce_dedupe_bucket_rows_padded returned (bucket * capacity + place, -1 = none); slots: device int64, batch b at
 * slots + b * slots_batch_stride: the cache slots this rank's owner-side cache op resolved for the rows requested
 * from it, requester-major.  A rank's request to ITSELF occupies places [local_lo, local_hi) = [rank * capacity,
 * (rank + 1) * capacity) on both sides, so for those places index_out = slots[b][pos] (the row is read and updated
 * in the cache, it never passes the exchange buffers); every other place p >= 0 becomes tail_base + p, a row of the
 * receive buffer the caller keeps tail_base rows behind the cache's first row in the same allocation
 * (ce_cache_set_cache_weight), so ce_bag_forward / ce_bag_backward_sgd_presorted_src see ONE table of tail_base +
 * world * capacity rows.  At world 1 the sharded step is then the unsharded one.  No upstream counterpart (upstream
 * has no row-wise sharding of a cached table). */
int ce_exchange_local_index(const int64_t* pos, int64_t n_per_batch, int64_t n_batches, const int64_t* slots,
                            int64_t slots_batch_stride, int64_t local_lo, int64_t local_hi, int64_t tail_base,
                            int64_t* index_out, ce_stream_t stream);

/* Early / late split of the row-wise exchange (API 5).  The reference exchanges the KJT
 * synchronously before every forward (recsys/datasets/utils.py:20-54) and the pooled embeddings after it; row-wise
 * sharding (baselines/dlrm_main.py:715-716 is the only place the reference can select it) exchanges ROWS, and a row of
 * step t depends on step t-1 only if some rank looked it up in step t-1.  The owner of a shard sees every rank's
 * requests of a whole prefetch window when it plans the window, so it can tell the two kinds apart:
 *   serve: device int64 [world][n_batches][capacity] -- the local rows peer w asks for in batch b (-1 = padding), as
 *          the id all-to-all of the window delivered them;
 *   prev / n_prev: the rows ANY peer asked for in the LAST batch of the window trained before this one (-1 entries
 *          are ignored), or NULL / 0 when no window precedes (then batch 0 depends on nothing in flight);
 *   mask:  scratch, device uint64 [n_local_rows], all zero on entry and all zero again on return;
 *   flags_out: device uint8, same shape as serve: bit 0 = LATE (requested by any peer in the batch before: the row
 *          must leave after that step's update has been applied), bit 1 = URGENT (requested by any peer in the batch
 *          after: the gradient returned for it must be applied before that step's late rows leave).  The last batch
 *          of the window is all URGENT (the next window is not planned yet).  Three launches, no host wait. */
int ce_split_classify(const int64_t* serve, int32_t world, int32_t n_batches, int64_t capacity, int64_t n_local_rows,
                      const int64_t* prev, int64_t n_prev, uint64_t* mask, uint8_t* flags_out, ce_stream_t stream);

/* Places of a window's requests inside the split exchange buffers (API 5), identical on both sides of the exchange:
 * the requester calls it on its requests and the flags the owners sent back, the owner on what it serves and its own
 * flags -- both batch-major, device int64 / uint8 [n_batches][world][capacity].  caps: device int32 [n_batches][4] =
 * {cap_early, cap_late, cap_deferred, cap_urgent} of every batch (the fixed message sizes of that step, rows per peer).
 * place_fwd (device int32, same shape): an EARLY row of peer w gets w * cap_early + its rank among the chunk's early
 * rows, a LATE row world * cap_early + w * cap_late + its rank among the late ones; an early row that does not fit
 * cap_early is placed behind the chunk's late rows (a row may always be sent later).  place_bwd the same with
 * DEFERRED (= not urgent) first.  Entries of peer `skip_peer` (a rank's requests to itself never travel: -1 = none),
 * padding and rows that fit nowhere get -1; the latter also set *overflow_flag (device int32, OR-ed): the caller
 * re-plans that window on the variable-size path.  counts_out (optional): device int32 [n_batches][world][4] = rows
 * classified {early, late, deferred, urgent} per chunk, for choosing the capacities. */
int ce_split_places(const int64_t* ids, const uint8_t* flags, int32_t n_batches, int32_t world, int64_t capacity,
                    int32_t skip_peer, const int32_t* caps, int32_t* place_fwd, int32_t* place_bwd,
                    int32_t* counts_out, int32_t* overflow_flag, ce_stream_t stream);

/* ce_exchange_local_index for the split exchange (API 5): TWO indices per lookup, one into "cache + forward buffers"
 * for the pooling, one into "cache + backward buffers" for the fused fold + SGD.  Behind the cache (tail_base rows
 * from its first row, one allocation: ce_cache_set_cache_weight) lie [E0 | E1 | L] -- n_early, n_early, n_late rows:
 * the early region exists twice because a step's early rows arrive while the step before still pools from its own,
 * batch b uses copy b & 1 -- and, bwd_base rows further, [D0 | U | D1] (n_deferred, n_urgent, n_deferred rows: with U
 * between the two deferred copies a step's fold writes ONE contiguous range, which is what is zeroed before it).
 * Places in [local_lo, local_hi) (this rank's own chunk) become the cache slot in both indices. */
int ce_exchange_local_index_split(const int64_t* pos, int64_t n_per_batch, int64_t n_batches, const int64_t* slots,
                                  const int32_t* place_fwd, const int32_t* place_bwd, int64_t chunk_stride,
                                  int64_t local_lo, int64_t local_hi, int64_t tail_base, int64_t bwd_base,
                                  const int32_t* caps, int32_t world, int64_t n_early, int64_t n_urgent,
                                  int64_t n_deferred, int64_t* index_fwd, int64_t* index_bwd, ce_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The F.embedding_bag arguments the reference forwards (recsys/models/dlrm.py:99-110 -> upstream A.7) and none of its
 * scripts sets (API 3).  Plain kernels (any dim, one wave per bag / row), off the benchmarked path.
 *
 * mode = 'max': out[bag][d] = max over the bag's rows (0 for a bag without valid rows), written like ce_bag_forward
 * (hook_features folds the shape hook).  max_pos (device int32 [num_bags, dim], may be NULL for inference) receives the
 * lookup that supplied each maximum (-1: none; the first of equal maxima, as torch's CPU kernel).  ce_bag_backward_max
 * routes the gradient there: dst[indices[max_pos[bag][d]]][d] += alpha * grad_out[bag][d] -- alpha 1 into a zeroed
 * grad_weight, alpha -lr straight into the weight (fused SGD). */
int ce_bag_forward_max(const float* weight, int64_t num_rows, int32_t dim, const int64_t* indices, int64_t nnz,
                       const void* offsets, int32_t offsets_are_i64, int64_t num_bags, int32_t include_last_offset,
                       int64_t hook_features, float* out, int32_t* max_pos, ce_stream_t stream);
int ce_bag_backward_max(float* dst, int64_t num_rows, int32_t dim, const int64_t* indices, int64_t nnz,
                        int64_t num_bags, int64_t hook_features, const float* grad_out, const int32_t* max_pos,
                        float alpha, ce_stream_t stream);
/* Gradient w.r.t. per_sample_weights (mode 'sum'): grad_psw[j] = < grad_out[bag of j], weight[indices[j]] >, 0 for an
 * ignored lookup.  grad_psw: device fp32 [nnz]. */
int ce_bag_backward_psw(const float* weight, int64_t num_rows, int32_t dim, const int64_t* indices, int64_t nnz,
                        const void* offsets, int32_t offsets_are_i64, int64_t num_bags, int32_t include_last_offset,
                        int64_t hook_features, const float* grad_out, float* grad_psw, ce_stream_t stream);
/* max_norm / norm_type (torch.embedding_renorm_, applied by F.embedding_bag before the lookup): every row an index
 * names is scaled by max_norm / (norm + 1e-7) if its norm_type-norm exceeds max_norm -- once, however often it is named.
 * workspace: device memory of ce_rows_renorm_workspace(num_rows) bytes (a bitmap of the named rows). */
size_t ce_rows_renorm_workspace(int64_t num_rows);
int ce_rows_renorm(float* weight, int64_t num_rows, int32_t dim, const int64_t* indices, int64_t n, float max_norm,
                   float norm_type, void* workspace, size_t workspace_bytes, ce_stream_t stream);

/* weight[index[i]] += alpha * src_rows[i] for i < n (whole rows of `dim` floats; repeated / out-of-range
 * index entries are summed / skipped).  Owner-side update of the row-wise exchange: the requester has
 * already folded a batch's duplicates, so each received gradient row is applied as is (alpha = -lr). */
int ce_rows_axpy(float* weight, int64_t num_rows, int32_t dim, const int64_t* index, int64_t n,
                 const float* src_rows, float alpha, ce_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CE_API_H */
