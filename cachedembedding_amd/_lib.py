"""ctypes binding of libce_hip.so (the C ABI in include/ce_api.h).

There is deliberately no CPU fallback: if the HIP library is missing or cannot be loaded
the import fails loudly.  torch is imported first so the library binds to the HIP runtime
(libamdhip64.so.7) that torch already mapped -- device pointers of torch tensors and the
current torch stream are then valid arguments for every entry point.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p
from pathlib import Path

import torch  # noqa: F401  (must precede the CDLL below)

_PKG = Path(__file__).resolve().parent
# CE_LIBRARY: another build of the same sources (tests load libce_hip_testhooks.so, the -DCE_TEST_HOOKS twin, this way)
LIB_PATH = Path(os.environ["CE_LIBRARY"]) if os.environ.get("CE_LIBRARY") else _PKG / "libce_hip.so"

CE_OK = 0
CE_ERR_INVALID = 1
CE_ERR_HIP = 2
CE_ERR_CAPACITY = 3
CE_ERR_NOMEM = 4
CE_ERR_UNSUPPORTED = 5
CE_ERR_RANGE = 6
CE_EVICT_DATASET = 0
CE_EVICT_LFU = 1
CE_EVICT_LRU = 2
CE_MODE_SUM = 0
CE_MODE_MEAN = 1
CE_ACT_F32 = 0
CE_ACT_BF16 = 1
CE_ACT_F16 = 2
CE_OPT_SGD = 0
CE_OPT_ROWWISE_ADAGRAD = 1
CE_ROUND_NEAREST = 0
CE_ROUND_STOCHASTIC = 1
CE_SORTED_CHUNK = 64
CE_COMPACT_BLOCK = 4096
CE_ACC_CACHE = 0
CE_ACC_STEP = 1
CE_WD_NONE = 0
CE_WD_L2 = 1
CE_WD_DECOUPLED = 2
CE_CLIP_NONE = 0
CE_CLIP_VALUE = 1
CE_CLIP_ROW_NORM = 2
CE_TRANSPORT_ZEROCOPY = 0
CE_TRANSPORT_STAGED = 1
CE_TRANSPORT_WORKER = 2
CE_CALL_PREPARE = 0
CE_CALL_PRELOAD = 1
CE_CALL_FLUSH = 2
CE_Q8_HEADER_BYTES = 16
CE_Q4_HEADER_BYTES = 16


class CeCacheConfig(Structure):
    _fields_ = [
        ("num_embeddings", c_int64),
        ("cuda_row_num", c_int64),
        ("embedding_dim", c_int32),
        ("evict_strategy", c_int32),
        ("transport", c_int32),
        ("protect_depth", c_int32),
        ("max_ids_per_call", c_int64),
        ("host_weight", c_void_p),
        ("host_weight_dev", c_void_p),
        ("cache_weight", c_void_p),
        ("idx_map", c_void_p),
        ("inverted_cached_idx", c_void_p),
        ("cached_idx_map", c_void_p),
        ("freq_cnter", c_void_p),
        ("workspace", c_void_p),
        ("workspace_bytes", c_size_t),
    ]


class CeCallStats(Structure):
    _fields_ = [
        ("seq", c_int64),
        ("n_ids", c_int64),
        ("n_unique", c_int64),
        ("n_miss", c_int64),
        ("n_evict", c_int64),
        ("miss_lookups", c_int64),
        ("n_free_after", c_int64),
        ("status", c_int32),
        ("kind", c_int32),
    ]


# name -> (restype, argtypes); mirrors include/ce_api.h declaration by declaration (tests/test_abi.py compares the two
# parameter by parameter).  The groups the ce_bag_* declarations are made of, each written once and in the order the
# lists have them -- functional._fused_update_call builds the argument tuples from the same ones:
_ROWS = [c_int64, c_int32]                      # num_rows, dim
_TABLE = [c_void_p] + _ROWS                     # the table in front of them
_TABLE_W16 = [c_void_p, c_int32] + _ROWS        # ... with its CE_ACT_* code: the entries a 16-bit table goes to
# indices, nnz, offsets, offsets_are_i64, num_bags, include_last_offset
_SLOTS = [c_void_p, c_int64, c_void_p, c_int32, c_int64, c_int32]
_POOL = [c_void_p, c_int32, c_int64, c_void_p]  # per_sample_weights, mode, hook_features, out / grad_out
_LOOKUPS = _TABLE + _SLOTS
_BAG = _LOOKUPS + _POOL                         # the slots + offsets entries
_BAG_W16 = _TABLE_W16 + _SLOTS + _POOL
_SRC_WALK = [c_int64, c_void_p]                 # nnz, grad_out: the backward entries that walk source-row keys
_SRC = _TABLE + _SRC_WALK
_SRC_W16 = _TABLE_W16 + _SRC_WALK
_ACT = [c_int32]                # act_dtype, right behind the out / grad_out it describes
_KEYS = [c_void_p]              # presorted / source-row keys
_ROW_STATE = [c_void_p, c_void_p, c_int64]      # row_of_slot, momentum (partial row-wise Adam: v), its rows
_RATE = [c_float, c_float]                      # lr, eps
_RATE_DEV = [c_void_p, c_float]                 # lr as ONE fp32 in device memory, eps
_RATE_BOTH = [c_float, c_void_p, c_float]       # lr, lr_dev, eps
_BETAS = [c_double, c_double]                   # beta1, beta2
_LR_DECAY = [c_double]                          # element-wise Adagrad: lr_decay where Adam has its betas
_WD = [c_float, c_int32]                        # weight_decay, weight_decay_mode: directly behind eps
_CLIP = [c_float, c_int32]                      # grad_clip, grad_clip_mode: directly behind weight_decay_mode
_OPT = [c_int32, c_int32, c_uint64]             # optimizer, rounding, seed
_STEP = [c_void_p]                              # the in-row layouts' step count on the device
_ACC = [c_int32]                                # accumulator (CE_ACC_*)
_STREAM = [c_void_p]
_WS = [c_void_p, c_size_t] + _STREAM            # workspace, workspace_bytes, stream
# row-wise Adagrad and SGD with a per-row pass, behind the lookups and their act_dtype: the sorted entries take no keys
_ADAGRAD_TAIL = _KEYS + _ROW_STATE + _RATE + _WS
_UPDATE_SORTED_TAIL = _ROW_STATE + _RATE + _OPT + _WS
_UPDATE_TAIL = _KEYS + _UPDATE_SORTED_TAIL
_LRDEV_TAIL = _KEYS + _ROW_STATE + _RATE_DEV + _OPT + _ACC + _WS
_UPDATE_WD_TAIL = _KEYS + _ROW_STATE + _RATE_BOTH + _WD + _OPT + _ACC + _WS
_UPDATE_CLIP_TAIL = _KEYS + _ROW_STATE + _RATE_BOTH + _WD + _CLIP + _OPT + _ACC + _WS
_SORTED_WD_TAIL = _ROW_STATE + _RATE + _WD + _OPT + _WS
_SORTED_CLIP_TAIL = _ROW_STATE + _RATE + _WD + _CLIP + _OPT + _WS
# the in-row layouts behind their moments (beta1, beta2 or lr_decay), which stand behind the keys -- partial row-wise
# Adam: behind keys and row state; the sorted entries: no keys, no accumulator
_IN_ROW_TAIL = _RATE_BOTH + _STEP + _ACC + _WS
_IN_ROW_WD_TAIL = _RATE_BOTH + _WD + _STEP + _ACC + _WS
_IN_ROW_CLIP_TAIL = _RATE_BOTH + _WD + _CLIP + _STEP + _ACC + _WS
_IN_ROW_SORTED_TAIL = _RATE_BOTH + _WD + _CLIP + _STEP + _WS
# the window presort: slots, nnz_per_batch, n_batches, num_rows | offsets, offsets_are_i64, offsets_batch_stride,
# num_bags, include_last_offset, hook_features
_WINDOW = [c_void_p, c_int64, c_int64, c_int64]
_WINDOW_SRC = _WINDOW + [c_void_p, c_int32, c_int64, c_int64, c_int32, c_int64]
SIGNATURES = {
    "ce_version": (c_int, []),
    "ce_cpu_budget": (c_int32, []),
    "ce_last_error": (c_char_p, []),
    "ce_stream_create_cu_mask": (c_int, [c_void_p, c_int32, POINTER(c_void_p)]),
    "ce_stream_destroy": (c_int, [c_void_p]),
    "ce_host_alloc": (c_int, [c_size_t, c_int, POINTER(c_void_p), POINTER(c_void_p)]),
    "ce_host_free": (c_int, [c_void_p]),
    "ce_host_register": (c_int, [c_void_p, c_size_t, POINTER(c_void_p)]),
    "ce_host_unregister": (c_int, [c_void_p]),
    "ce_host_fill_uniform": (c_int, [c_void_p, c_int64, c_float, c_float, c_uint64, c_int]),
    "ce_host_fill_uniform_rows": (c_int, [c_void_p, c_int64, c_int32, c_float, c_float, c_uint64, c_void_p, c_void_p]),
    "ce_host_rows_gather": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    "ce_box_probe": (c_int, [c_void_p, c_size_t, c_int32, POINTER(c_double), POINTER(c_double), c_void_p]),
    "ce_probe_rows": (c_int, [c_void_p, c_int64, c_int32, c_int64, c_int32, POINTER(c_double), POINTER(c_double), c_void_p]),
    "ce_bag_forward": (c_int, _BAG + _STREAM),
    "ce_bag_backward_dense": (c_int, _BAG + _STREAM),
    "ce_bag_backward_dense_presorted": (c_int, _BAG + _KEYS + _STREAM),
    "ce_bag_backward_rows": (c_int, [c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_int32, c_int64, c_int32, c_void_p,
                                     c_int32, c_int64, c_void_p, c_void_p]),
    "ce_bag_backward_sgd": (c_int, _BAG + [c_float] + _STREAM),
    "ce_bag_presort_len": (c_int64, [c_int64]),
    "ce_bag_presort": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "ce_bag_backward_sgd_presorted": (c_int, _BAG + [c_float] + _KEYS + _STREAM),
    "ce_bag_presort_window": (c_int, _WINDOW + _KEYS + _STREAM),
    "ce_bag_presort_window_src": (c_int, _WINDOW_SRC + _KEYS + _STREAM),
    "ce_bag_forward_src_keys": (c_int, _TABLE + [c_int64] + _KEYS + [c_void_p] + _STREAM),
    "ce_bag_backward_sgd_presorted_src": (c_int, _SRC + [c_float] + _KEYS + _STREAM),
    # ... ids, keys_out, seg_id_ranges
    "ce_bag_presort_window_src_excl": (c_int, _WINDOW_SRC + [c_void_p] + _KEYS + [c_void_p] + _STREAM),
    "ce_bag_backward_sgd_presorted_src_excl": (c_int, _SRC + [c_float] + _KEYS + [c_void_p] + _STREAM),
    "ce_bag_backward_dense_presorted_src": (c_int, _SRC + _KEYS + _STREAM),
    "ce_bag_backward_sgd_sorted_workspace": (c_size_t, [c_int64, c_int64]),
    "ce_bag_backward_sgd_sorted": (c_int, _BAG + [c_float, c_void_p, c_size_t] + _STREAM),
    "ce_bag_backward_rowwise_adagrad_workspace": (c_size_t, [c_int64, c_int32]),
    "ce_bag_backward_rowwise_adagrad": (c_int, _BAG + _ADAGRAD_TAIL),
    "ce_bag_backward_rowwise_adagrad_src": (c_int, _SRC + _ADAGRAD_TAIL),
    # the hot-path bag entries with the output / incoming gradient as void* of an activation dtype (CE_ACT_*)
    "ce_bag_forward_act": (c_int, _BAG + _ACT + _STREAM),
    "ce_bag_forward_src_keys_act": (c_int, _TABLE + [c_int64] + _KEYS + [c_void_p] + _ACT + _STREAM),
    "ce_bag_backward_dense_act": (c_int, _BAG + _ACT + _KEYS + _STREAM),
    "ce_bag_backward_sgd_act": (c_int, _BAG + _ACT + [c_float] + _KEYS + _STREAM),
    "ce_bag_backward_sgd_src_act": (c_int, _SRC + _ACT + [c_float] + _KEYS + [c_void_p] + _STREAM),
    "ce_bag_backward_dense_src_act": (c_int, _SRC + _ACT + _KEYS + _STREAM),
    "ce_bag_backward_rowwise_adagrad_act": (c_int, _BAG + _ACT + _ADAGRAD_TAIL),
    "ce_bag_backward_rowwise_adagrad_src_act": (c_int, _SRC + _ACT + _ADAGRAD_TAIL),
    # 16-bit table: weight, weight_dtype in front; the update's tail = keys, row_of_slot, momentum, momentum_rows, lr,
    # eps, optimizer, rounding, seed, workspace, workspace_bytes, stream
    "ce_host_fill_uniform_w16": (c_int, [c_void_p, c_int64, c_float, c_float, c_uint64, c_int32, c_int]),
    "ce_bag_forward_w16": (c_int, _BAG_W16 + _ACT + _STREAM),
    "ce_bag_forward_src_keys_w16": (c_int, _TABLE_W16 + [c_int64] + _KEYS + [c_void_p] + _ACT + _STREAM),
    "ce_bag_backward_w16_workspace": (c_size_t, [c_int64, c_int32]),
    "ce_bag_backward_update_w16": (c_int, _BAG_W16 + _ACT + _UPDATE_TAIL),
    "ce_bag_backward_update_src_w16": (c_int, _SRC_W16 + _ACT + _UPDATE_TAIL),
    # the deterministic, accumulator-free update: the w16 update's arguments without the presorted keys
    "ce_bag_backward_update_sorted_workspace": (c_size_t, [c_int64, c_int64, c_int32]),
    "ce_bag_backward_update_sorted": (c_int, _BAG_W16 + _ACT + _UPDATE_SORTED_TAIL),
    # the atomic updates with a step-sized accumulator: the w16 update's arguments, weight_dtype may be CE_ACT_F32
    "ce_bag_backward_update_compact_workspace": (c_size_t, [c_int64, c_int64, c_int32]),
    "ce_bag_backward_update_compact": (c_int, _BAG_W16 + _ACT + _UPDATE_TAIL),
    "ce_bag_backward_update_compact_src": (c_int, _SRC_W16 + _ACT + _UPDATE_TAIL),
    # the learning rate as ONE fp32 in device memory, read by the kernels when they run: the _act / _w16 lists with lr a
    # pointer; the update pair also takes the accumulator (CE_ACC_*) behind the seed and covers the cache-sized fp32
    # Adagrad, the cache-sized 16-bit and the step-sized entries
    "ce_bag_backward_sgd_lrdev": (c_int, _BAG + _ACT + [c_void_p] + _KEYS + _STREAM),
    "ce_bag_backward_sgd_src_lrdev": (c_int, _SRC + _ACT + [c_void_p] + _KEYS + [c_void_p] + _STREAM),
    "ce_bag_backward_update_lrdev": (c_int, _BAG_W16 + _ACT + _LRDEV_TAIL),
    "ce_bag_backward_update_src_lrdev": (c_int, _SRC_W16 + _ACT + _LRDEV_TAIL),
    # the Adam-layout table (rows w | m | v of 3 * dim fp32): the fp32 forwards' lists; the update's tail = keys, beta1,
    # beta2, lr, lr_dev, eps, step, accumulator, workspace, workspace_bytes, stream
    "ce_host_fill_uniform_adam": (c_int, [c_void_p, c_int64, c_int32, c_float, c_float, c_uint64, c_int]),
    "ce_bag_forward_adam": (c_int, _BAG + _ACT + _STREAM),
    "ce_bag_forward_src_keys_adam": (c_int, _TABLE + [c_int64] + _KEYS + [c_void_p] + _ACT + _STREAM),
    "ce_bag_backward_adam_workspace": (c_size_t, [c_int64, c_int64, c_int32, c_int32]),
    "ce_bag_backward_adam": (c_int, _BAG + _ACT + _KEYS + _BETAS + _IN_ROW_TAIL),
    "ce_bag_backward_adam_src": (c_int, _SRC + _ACT + _KEYS + _BETAS + _IN_ROW_TAIL),
    # weight decay (L2 / decoupled, lazy) for the fused updates: the covered lists with the decay behind eps
    "ce_bag_backward_update_wd": (c_int, _BAG_W16 + _ACT + _UPDATE_WD_TAIL),
    "ce_bag_backward_update_src_wd": (c_int, _SRC_W16 + _ACT + _UPDATE_WD_TAIL),
    "ce_bag_backward_update_sorted_wd": (c_int, _BAG_W16 + _ACT + _SORTED_WD_TAIL),
    "ce_bag_backward_adam_wd": (c_int, _BAG + _ACT + _KEYS + _BETAS + _IN_ROW_WD_TAIL),
    "ce_bag_backward_adam_src_wd": (c_int, _SRC + _ACT + _KEYS + _BETAS + _IN_ROW_WD_TAIL),
    # partial row-wise Adam (rows w | m of 2 * dim fp32, the second moment one fp32 per table row): the Adam layout's
    # lists; the update's = the _adam_wd lists with row_of_slot, v, v_rows behind the keys
    "ce_host_fill_uniform_pradam": (c_int, [c_void_p, c_int64, c_int32, c_float, c_float, c_uint64, c_int]),
    "ce_bag_forward_pradam": (c_int, _BAG + _ACT + _STREAM),
    "ce_bag_forward_src_keys_pradam": (c_int, _TABLE + [c_int64] + _KEYS + [c_void_p] + _ACT + _STREAM),
    "ce_bag_backward_pradam_workspace": (c_size_t, [c_int64, c_int64, c_int32, c_int32]),
    "ce_bag_backward_pradam": (c_int, _BAG + _ACT + _KEYS + _ROW_STATE + _BETAS + _IN_ROW_WD_TAIL),
    "ce_bag_backward_pradam_src": (c_int, _SRC + _ACT + _KEYS + _ROW_STATE + _BETAS + _IN_ROW_WD_TAIL),
    # gradient clipping (per value / per row norm) for the fused updates: the covered lists with the clip behind the decay
    "ce_bag_backward_update_clip": (c_int, _BAG_W16 + _ACT + _UPDATE_CLIP_TAIL),
    "ce_bag_backward_update_src_clip": (c_int, _SRC_W16 + _ACT + _UPDATE_CLIP_TAIL),
    "ce_bag_backward_update_sorted_clip": (c_int, _BAG_W16 + _ACT + _SORTED_CLIP_TAIL),
    "ce_bag_backward_adam_clip": (c_int, _BAG + _ACT + _KEYS + _BETAS + _IN_ROW_CLIP_TAIL),
    "ce_bag_backward_adam_src_clip": (c_int, _SRC + _ACT + _KEYS + _BETAS + _IN_ROW_CLIP_TAIL),
    "ce_bag_backward_pradam_clip": (c_int, _BAG + _ACT + _KEYS + _ROW_STATE + _BETAS + _IN_ROW_CLIP_TAIL),
    "ce_bag_backward_pradam_src_clip": (c_int, _SRC + _ACT + _KEYS + _ROW_STATE + _BETAS + _IN_ROW_CLIP_TAIL),
    # element-wise Adagrad (rows w | h of 2 * dim fp32, h the per-element sums of squares): the partial row-wise Adam
    # forwards' lists; the fill's list with init_acc in front of threads
    "ce_host_fill_uniform_adagrad": (c_int, [c_void_p, c_int64, c_int32, c_float, c_float, c_uint64, c_float, c_int]),
    "ce_bag_forward_adagrad": (c_int, _BAG + _ACT + _STREAM),
    "ce_bag_forward_src_keys_adagrad": (c_int, _TABLE + [c_int64] + _KEYS + [c_void_p] + _ACT + _STREAM),
    "ce_bag_backward_adagrad_workspace": (c_size_t, [c_int64, c_int64, c_int32, c_int32]),
    "ce_bag_backward_adagrad": (c_int, _BAG + _ACT + _KEYS + _LR_DECAY + _IN_ROW_CLIP_TAIL),
    "ce_bag_backward_adagrad_src": (c_int, _SRC + _ACT + _KEYS + _LR_DECAY + _IN_ROW_CLIP_TAIL),
    # the deterministic, accumulator-free updates of the three in-row layouts: slots + offsets, no keys, no accumulator
    "ce_bag_backward_in_row_sorted_workspace": (c_size_t, [c_int64, c_int64, c_int32]),
    "ce_bag_backward_adam_sorted": (c_int, _BAG + _ACT + _BETAS + _IN_ROW_SORTED_TAIL),
    "ce_bag_backward_pradam_sorted": (c_int, _BAG + _ACT + _ROW_STATE + _BETAS + _IN_ROW_SORTED_TAIL),
    "ce_bag_backward_adagrad_sorted": (c_int, _BAG + _ACT + _LR_DECAY + _IN_ROW_SORTED_TAIL),
    # the 8-bit row-wise quantized table (q8): rows of 16 + dim bytes; forward only
    "ce_q8_row_bytes": (c_size_t, [c_int32]),
    "ce_host_quantize_q8": (c_int, [c_void_p, c_int32, c_int64, c_int32, c_void_p, c_int]),
    "ce_host_dequantize_q8": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int]),
    "ce_bag_forward_q8": (c_int, _BAG + _ACT + _STREAM),
    "ce_bag_forward_src_keys_q8": (c_int, _TABLE + [c_int64] + _KEYS + [c_void_p] + _ACT + _STREAM),
    # the 4-bit row-wise quantized table (q4): rows of 16 + dim / 2 bytes; the q8 entries' argument lists
    "ce_q4_row_bytes": (c_size_t, [c_int32]),
    "ce_host_quantize_q4": (c_int, [c_void_p, c_int32, c_int64, c_int32, c_void_p, c_int]),
    "ce_host_dequantize_q4": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int]),
    "ce_bag_forward_q4": (c_int, _BAG + _ACT + _STREAM),
    "ce_bag_forward_src_keys_q4": (c_int, _TABLE + [c_int64] + _KEYS + [c_void_p] + _ACT + _STREAM),
    # the device-side quantizer of both formats: src, src_dtype, n_rows, dim, dst, first_bad, stream
    "ce_quantize_rows_q8": (c_int, [c_void_p, c_int32, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "ce_quantize_rows_q4": (c_int, [c_void_p, c_int32, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "ce_cache_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int32]),
    "ce_cache_create": (c_int, [POINTER(CeCacheConfig), c_void_p, POINTER(c_void_p)]),
    "ce_cache_destroy": (c_int, [c_void_p]),
    "ce_cache_preload": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "ce_cache_set_freq_bound": (c_int, [c_void_p, c_int64]),
    "ce_cache_prepare_ids": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "ce_cache_prepare_ids_keys": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int32, c_void_p, c_int32,
                                          c_int64, c_int64, c_int32, c_int64, c_void_p, c_void_p]),
    "ce_cache_prepare_ids_begin": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int32, c_void_p, c_int32,
                                           c_int64, c_int64, c_int32, c_int64, c_void_p, c_void_p]),
    "ce_cache_prepare_ids_finish": (c_int, [c_void_p, c_void_p]),
    "ce_cache_prepare_ids_padded": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "ce_cache_prepare_ids_begin_padded": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "ce_cache_set_deferred_rows": (c_int, [c_void_p, c_int32]),
    "ce_cache_rows_ticket": (c_int64, [c_void_p]),
    "ce_cache_wait_rows": (c_int, [c_void_p, c_int64, c_void_p]),
    "ce_cache_last_stats": (c_int, [c_void_p, POINTER(CeCallStats)]),
    "ce_cache_totals": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64),
                                POINTER(c_int64), POINTER(c_int64)]),
    "ce_cache_history": (c_int64, [c_void_p, c_int64, POINTER(CeCallStats), c_int64]),
    "ce_cache_lookup_slots": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "ce_cache_flush": (c_int, [c_void_p, c_void_p]),
    "ce_cache_install_rows": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "ce_cache_set_protect_depth": (c_int, [c_void_p, c_int32]),
    "ce_cache_set_transport": (c_int, [c_void_p, c_int32]),
    "ce_cache_get_transport": (c_int32, [c_void_p]),
    "ce_cache_set_cache_weight": (c_int, [c_void_p, c_void_p]),
    "ce_cache_graph_replayed": (c_int, [c_void_p, c_int64, c_int64, c_void_p]),
    "ce_cache_set_buffer_rows": (c_int, [c_void_p, c_int64]),
    "ce_cache_set_profiling": (c_int, [c_void_p, c_int32]),
    "ce_cache_phase_count": (c_int32, []),
    "ce_cache_phase_name": (c_char_p, [c_int32]),
    "ce_cache_phase_times": (c_int, [c_void_p, POINTER(c_double), c_int32, POINTER(c_int64), c_int32]),
    "ce_cache_writeback_wait": (c_int, [c_void_p]),
    "ce_cache_swap_stats": (c_int, [c_void_p, POINTER(c_double), POINTER(c_int64)]),
    "ce_cache_failures": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int32), POINTER(c_int64)]),
    "ce_cache_free_rows": (c_int, [c_void_p, POINTER(c_int64)]),
    "ce_bucketize_workspace": (c_size_t, [c_int64, c_int32]),
    "ce_bucketize_rows": (c_int, [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_size_t, c_void_p]),
    "ce_dedupe_bucket_rows": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ce_dedupe_bucket_rows_padded": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int64, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ce_dedupe_bucket_rows_padded_window": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int32, c_int64,
                                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                    c_void_p, c_void_p]),
    "ce_exchange_local_index": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64,
                                        c_void_p, c_void_p]),
    "ce_split_classify": (c_int, [c_void_p, c_int32, c_int32, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                  c_void_p]),
    "ce_split_places": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int64, c_int32, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    "ce_exchange_local_index_split": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                              c_int64, c_int64, c_int64, c_void_p, c_int32, c_int64, c_int64, c_int64,
                                              c_void_p, c_void_p, c_void_p]),
    "ce_bag_forward_max": (c_int, _LOOKUPS + [c_int64, c_void_p, c_void_p] + _STREAM),
    "ce_bag_backward_max": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                    c_float, c_void_p]),
    "ce_bag_backward_psw": (c_int, _LOOKUPS + [c_int64, c_void_p, c_void_p] + _STREAM),
    "ce_rows_renorm_workspace": (c_size_t, [c_int64]),
    "ce_rows_renorm": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_float, c_float, c_void_p, c_size_t,
                               c_void_p]),
    "ce_rows_axpy": (c_int, [c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_float, c_void_p]),
}


class CeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libce_hip error {code}: {msg}")
        self.code = code


def _load() -> ctypes.CDLL:
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback.")
    lib = ctypes.CDLL(str(LIB_PATH), mode=os.RTLD_NOW | os.RTLD_LOCAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError (loud) if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def last_error() -> str:
    m = lib.ce_last_error()
    return m.decode("utf-8", "replace") if m else ""


def check(rc: int) -> None:
    if rc != CE_OK:
        raise CeError(rc, last_error())


def require_gpu() -> None:
    if not torch.cuda.is_available():
        raise RuntimeError("cachedembedding_amd needs a HIP device (MI355X); no GPU is visible and there is "
                           "no CPU fallback for the product path")


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr() -> int:
    """hipStream_t of torch's current stream on the current device (the raw getter is ~20x cheaper than
    constructing a torch.cuda.Stream object, and this is called for every kernel launch)."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


# torch dtype of an activation tensor (or of a 16-bit table's rows) -> CE_ACT_*
ACT_DTYPES = {torch.float32: CE_ACT_F32, torch.bfloat16: CE_ACT_BF16, torch.float16: CE_ACT_F16}


def act_code(dtype) -> int:
    """CE_ACT_* of an output / gradient dtype; None means fp32.  Anything else is refused by name."""
    if dtype is None:
        return CE_ACT_F32
    try:
        return ACT_DTYPES[dtype]
    except (KeyError, TypeError):
        raise NotImplementedError(f"output_dtype={dtype!r}: torch.float32, torch.bfloat16 and torch.float16 are "
                                  "implemented") from None


W16_DTYPES = (torch.bfloat16, torch.float16)


def table_code(dtype) -> int:
    """CE_ACT_* of a table dtype (table_dtype=): None means fp32.  Anything else is refused by name."""
    if dtype is None:
        return CE_ACT_F32
    try:
        return ACT_DTYPES[dtype]
    except (KeyError, TypeError):
        raise NotImplementedError(f"table_dtype={dtype!r}: torch.float32, torch.bfloat16 and torch.float16 are "
                                  "implemented") from None


def check_w16_dim(dim: int) -> None:
    """a 16-bit table's rows are whole 16-byte units, one lane group per row: refused before the GPU is asked for"""
    if dim % 8 != 0 or dim > 1024 or dim <= 0:
        raise NotImplementedError(f"a 16-bit table needs embedding_dim % 8 == 0 and embedding_dim <= 1024 (got {dim})")


# the 8-bit row-wise quantized table (q8) is spelled torch.uint8: a [N, 16 + D] tensor of whole rows
Q8 = torch.uint8


def check_q8_dim(dim: int) -> None:
    """a q8 row is 16 + dim bytes, whole 16-byte units with 16-byte aligned codes: refused before the GPU is asked for"""
    if dim % 16 != 0 or dim < 16 or dim > 1024:
        raise NotImplementedError(f"a q8 (torch.uint8) table needs embedding_dim % 16 == 0 and 16 <= embedding_dim <= 1024 "
                                  f"(got {dim})")


def refuse_q8(what: str, table_dtype) -> None:
    """the classes a q8 table is not wired into refuse it by name, before the GPU is asked for"""
    if table_dtype == Q8:
        raise NotImplementedError(f"{what} with a q8 (torch.uint8) table: a quantized table is served by a single-process "
                                  "CachedEmbeddingBag (from_pretrained(..., table_dtype=torch.uint8) or quantized())")


def q8_row_bytes(dim: int) -> int:
    check_q8_dim(dim)
    return CE_Q8_HEADER_BYTES + dim


# the 4-bit row-wise quantized table (q4) is SPELLED torch.quint4x2 where a table_dtype is given; its storage is a
# [N, 16 + D / 2] torch.uint8 tensor of whole rows (nothing allocates a quint4x2 tensor).  A uint8 tensor's width cannot
# tell the two formats apart, so whoever holds q4 rows carries quant_bits = 4 beside them; torch.uint8 alone means q8.
Q4 = torch.quint4x2


def check_q4_dim(dim: int) -> None:
    """a q4 row is 16 + dim / 2 bytes, whole 16-byte units with 16-byte aligned codes: refused before the GPU is asked for"""
    if dim % 32 != 0 or dim < 32 or dim > 1024:
        raise NotImplementedError(f"a q4 (torch.quint4x2) table needs embedding_dim % 32 == 0 and 32 <= embedding_dim <= "
                                  f"1024 (got {dim})")


def refuse_q4(what: str, table_dtype) -> None:
    """refuse_q8 for a q4 table"""
    if table_dtype == Q4:
        raise NotImplementedError(f"{what} with a q4 (torch.quint4x2) table: a quantized table is served by a "
                                  "single-process CachedEmbeddingBag (from_pretrained(..., table_dtype=torch.quint4x2) or "
                                  "quantized(bits=4))")


def refuse_quantized(what: str, table_dtype) -> None:
    refuse_q8(what, table_dtype)
    refuse_q4(what, table_dtype)


def q4_row_bytes(dim: int) -> int:
    check_q4_dim(dim)
    return CE_Q4_HEADER_BYTES + dim // 2


def quant_bits_of(table_dtype) -> int:
    """8 for a q8, 4 for a q4 table_dtype, 0 for any other"""
    return 8 if table_dtype == Q8 else (4 if table_dtype == Q4 else 0)


def check_quant_bits(bits) -> int:
    if bits not in (4, 8):
        raise NotImplementedError(f"quantized rows of {bits!r} bits: 8 (q8) and 4 (q4) are implemented")
    return bits


# the Adam layout (fused_optimizer="adam"): an fp32 table whose rows carry their moments, [N, 3 * D] = w | m | v
# partial row-wise Adam (fused_optimizer="partial_rowwise_adam"): [N, 2 * D] = w | m, the second moment one fp32 per row
# in device memory
# element-wise Adagrad (fused_optimizer="adagrad"): [N, 2 * D] = w | h, h the per-element sums of squared gradients
# 
LAYOUTS = (None, "adam", "partial_rowwise_adam", "adagrad")
LAYOUT_SPAN = {None: 1, "adam": 3, "partial_rowwise_adam": 2, "adagrad": 2}      # row parts of D floats
LAYOUT_NAMES = "None, 'adam', 'partial_rowwise_adam' or 'adagrad'"


def check_layout(layout):
    if layout not in LAYOUTS:
        raise ValueError(f"layout={layout!r}: {LAYOUT_NAMES}")
    return layout


def check_adam_dim(dim: int) -> None:
    """the three parts of an Adam-layout row are whole 16-byte units, one lane group per row: refused before the GPU is
    asked for"""
    if dim % 4 != 0 or dim < 4 or dim > 1024:
        raise NotImplementedError(f"an Adam-layout table needs embedding_dim % 4 == 0 and 4 <= embedding_dim <= 1024 "
                                  f"(got {dim})")


def check_adam_table(dim: int, table_dtype, layout: str = "adam") -> None:
    """what fused_optimizer="adam" / "partial_rowwise_adam" / "adagrad" needs of the table: fp32 rows (no 16-bit, no
    quantized table) and the dim rule"""
    if quant_bits_of(table_dtype) or table_code(table_dtype) != CE_ACT_F32:
        if layout == "adagrad":
            raise NotImplementedError(f"fused_optimizer={layout!r} with table_dtype={table_dtype}: a table whose rows "
                                      "carry their Adagrad state is an fp32 table (a 16-bit state or table is not "
                                      "implemented)")
        raise NotImplementedError(f"fused_optimizer={layout!r} with table_dtype={table_dtype}: the Adam layout is an "
                                  "fp32 table (16-bit moments or tables are not implemented)")
    check_adam_dim(dim)


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()
