"""CPU reference model of the LRU eviction strategy (CE_EVICT_LRU in include/ce_api.h): the oracle's
cache manager (oracle/cache_oracle.py, imported, not edited) with a per-slot last use and the LRU victim rule.

  last use   the number of the most recent prepare_ids call that named the slot's row (being admitted counts); 0 for a
             row the warm-up preload placed: never used, older than every use.  Only the order of the numbers matters.
  victims    the k eligible (resident, not protected) slots with the oldest last use; among equal last uses the HIGHER
             slot first -- lexsort over (last use ascending, slot descending).
  reorder    with a frequency mapping: the top ceil(C * warmup_ratio) rows by the canonical stable-descending order into
             slots 0..n-1 (the LFU preload without counters), idx_map stays the identity; without: rows 0..n-1.
  failed     a call that fails (bad id, more unique rows than C) changes no map and no row.  failed_call_is_use says
             whether it still counts as a use of the resident rows it named: True is the library's per-lookup front
             (every launched call), False its bitmap front (captured calls), which stamps nothing when a call fails.
  protect    protect_depth as the oracle has it: the rows of the previous `protect_depth` calls stay protected.  A
             failed call is a call: it ages the history, and protects what it used where it counts as a use.
"""
import math

import numpy as np

from oracle.cache_oracle import OracleCachedParamMgr

LRU = "lru"


class LruOracleCachedParamMgr(OracleCachedParamMgr):
    def __init__(self, weight, cuda_row_num, failed_call_is_use=True):
        super().__init__(weight, cuda_row_num, LRU)
        self.failed_call_is_use = failed_call_is_use
        self.last_use = np.zeros(self.cuda_row_num, dtype=np.int64)
        self.calls = 0

    def reorder(self, ids_freq_mapping=None, warmup_ratio=0.7):
        N, C = self.num_embeddings, self.cuda_row_num
        n = min(int(math.ceil(C * warmup_ratio)), N)
        if n <= 0:
            return
        rows = np.arange(n, dtype=np.int64)
        if ids_freq_mapping is not None:
            freq = np.asarray(ids_freq_mapping, dtype=np.int64)
            assert freq.shape == (N,)
            rows = np.argsort(-freq, kind="stable")[:n].astype(np.int64)
        slots = np.arange(n, dtype=np.int64)
        self.cuda_cached_weight[slots] = self.weight[rows]
        self.cached_idx_map[slots] = rows
        self.inverted_cached_idx[rows] = slots
        self.last_use[slots] = 0
        self.cuda_available_row_num -= n

    def eligible(self, protected_rows):
        return (self.cached_idx_map >= 0) & ~np.isin(self.cached_idx_map, protected_rows)

    def _find_evict_gpu_idxs(self, k, protected_rows):
        slots = np.arange(self.cuda_row_num, dtype=np.int64)
        order = np.lexsort((-slots, self.last_use))                 # (last use asc, slot desc)
        order = order[self.eligible(protected_rows)[order]]
        assert len(order) >= k, "fewer eligible slots than victims"
        return order[:k].astype(np.int64)

    def prepare_ids(self, ids):
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        self.calls += 1
        good = (ids >= 0) & (ids < self.num_embeddings)
        try:
            if not good.all():
                raise IndexError(f"an id is outside [0, {self.num_embeddings})")
            slots = super().prepare_ids(ids)        # (AssertionError before any change: more unique rows than C)
        except (IndexError, AssertionError):
            rows = np.unique(self.idx_map[ids[good]])
            used = rows[self.inverted_cached_idx[rows] >= 0] if self.failed_call_is_use else rows[:0]
            self.last_use[self.inverted_cached_idx[used]] = self.calls
            if self.protect_depth > 0:
                self._protect_history = (self._protect_history + [used.copy()])[-self.protect_depth:]
            raise
        self.last_use[np.unique(slots)] = self.calls
        return slots

    def prepare_ids_padded(self, ids):
        """the padded entries: -1 names nothing and gets slot -1 (the library's total of ids seen counts the call's
        length, padding included)"""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        pad = ids == -1
        out = np.full(ids.shape, -1, dtype=np.int64)
        out[~pad] = self.prepare_ids(ids[~pad])
        self.total_cache += int(pad.sum())
        return out

    def flush(self):
        super().flush()
        self.last_use[:] = 0
