"""host time per call of four ce_bag_* entries and two forms of the cache op, two builds of the library side by side in
one process:

    python profiles/probes/host_cost_ab.py <parent libce_hip.so> <a second copy of that file> <this build's libce_hip.so>

Measured as host_cost.py does -- bursts of calls into an empty queue, the clock stops before the sync -- at a shape that
keeps the GPU far from saturated (2048 x 13 lookups, D = 32; the cache op: ce_cache_prepare_ids on the zero-copy
transport and the ce_cache_prepare_ids_begin_padded + _finish pair on the worker transport, on a full cache of 100 k of
400 k rows, every call with ids of its own so that it misses and evicts; every measurement of these two makes a cache
of its own and destroys it, so that one swap engine is alive at a time -- with three alive the worker pair's time per
call follows the order in which the engines were created, whichever library: profiles/cache_host_refactor.md).  The
three libraries are loaded through ctypes under
different paths (so each is its own instance) and take turns call site by call site.  The yardstick is the parent
against its own copy (A/A): the branch passes if the median of its five rounds differs from the parent's by no more
than the largest A/A difference of a round.  Prints one JSON line per entry."""
import ctypes
import json
import os
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from cachedembedding_amd import _lib  # noqa: E402  (the signatures; its own library is not the one measured)


def load(path):
    lib = ctypes.CDLL(str(Path(path).resolve()), mode=os.RTLD_NOW | os.RTLD_LOCAL)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


class Cache:
    """one cache of library L on `transport`, filled until no slot is free"""

    def __init__(self, L, transport, ids, slots, sp, N=400_000, C=100_000, D=32):
        hp, dp = ctypes.c_void_p(), ctypes.c_void_p()
        assert L.ce_host_alloc(N * D * 4, 8, ctypes.byref(hp), ctypes.byref(dp)) == _lib.CE_OK, L.ce_last_error()
        self.L, self.host, self.ids, self.slots, self.sp, self.calls = L, hp, ids, slots, sp, 0
        self.arrays = [torch.zeros(C, D, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda"),
                       torch.empty(C, dtype=torch.int32, device="cuda")]
        n = ids.shape[1]
        ws = int(L.ce_cache_workspace_bytes(N, C, n, D))
        self.arrays.append(torch.empty(ws + 256, dtype=torch.uint8, device="cuda"))
        cfg = _lib.CeCacheConfig()
        cfg.num_embeddings, cfg.cuda_row_num, cfg.embedding_dim, cfg.max_ids_per_call = N, C, D, n
        cfg.evict_strategy, cfg.transport, cfg.protect_depth = _lib.CE_EVICT_DATASET, transport, 0
        cfg.host_weight, cfg.host_weight_dev = hp.value, dp.value
        cfg.cache_weight, cfg.inverted_cached_idx, cfg.cached_idx_map = (a.data_ptr() for a in self.arrays[:3])
        cfg.workspace, cfg.workspace_bytes = (self.arrays[3].data_ptr() + 255) & ~255, ws
        self.h = ctypes.c_void_p()
        assert L.ce_cache_create(ctypes.byref(cfg), sp, ctypes.byref(self.h)) == _lib.CE_OK, L.ce_last_error()
        self.split = transport == _lib.CE_TRANSPORT_WORKER
        free = ctypes.c_int64(-1)
        for _ in range(12):
            assert self.call() == _lib.CE_OK, L.ce_last_error()
        assert L.ce_cache_free_rows(self.h, ctypes.byref(free)) == _lib.CE_OK and free.value == 0, free.value

    def call(self):
        ids = self.ids[self.calls % self.ids.shape[0]].data_ptr()
        self.calls += 1
        n = self.ids.shape[1]
        if not self.split:
            return self.L.ce_cache_prepare_ids(self.h, ids, n, self.slots, self.sp)
        return (self.L.ce_cache_prepare_ids_begin_padded(self.h, ids, n, self.slots, self.sp)
                or self.L.ce_cache_prepare_ids_finish(self.h, self.sp))

    def close(self):
        self.L.ce_cache_destroy(self.h)
        self.L.ce_host_free(self.host)


def main():
    paths = sys.argv[1:4]
    assert len(paths) == 3 and len({str(Path(p).resolve()) for p in paths}) == 3, __doc__
    libs = dict(zip(("parent", "parent_copy", "branch"), (load(p) for p in paths)))
    torch.manual_seed(0)
    B, F, D, C = 2048, 13, 32, 100_000
    n = B * F
    dev = "cuda"
    w32 = torch.randn(C, D, device=dev)
    w16 = w32.to(torch.bfloat16)
    slots = torch.randint(0, C, (1, n), device=dev)
    off = torch.arange(n + 1, dtype=torch.int32, device=dev)
    klen = int(libs["parent"].ce_bag_presort_len(n))
    keys = torch.empty(1, klen, dtype=torch.int64, device=dev)
    out16 = torch.empty(B, F, D, dtype=torch.bfloat16, device=dev)
    grad = (torch.randn(B, F, D, device=dev) * 1e-3).to(torch.bfloat16)
    sp = _lib.stream_ptr()
    P = {k: v.data_ptr() for k, v in dict(w32=w32, w16=w16, slots=slots, off=off, keys=keys, out16=out16, grad=grad).items()}
    BF = _lib.CE_ACT_BF16
    entries = {
        "ce_bag_presort_window_src": lambda L: L.ce_bag_presort_window_src(P["slots"], n, 1, C, P["off"], 0, 0, n, 1, F,
                                                                           P["keys"], sp),
        "ce_bag_forward_src_keys_act": lambda L: L.ce_bag_forward_src_keys_act(P["w32"], C, D, n, P["keys"], P["out16"],
                                                                               BF, sp),
        "ce_bag_forward_w16": lambda L: L.ce_bag_forward_w16(P["w16"], BF, C, D, P["slots"], n, P["off"], 0, n, 1, None,
                                                             _lib.CE_MODE_SUM, F, P["out16"], BF, sp),
        "ce_bag_backward_sgd_src_act": lambda L: L.ce_bag_backward_sgd_src_act(P["w32"], C, D, n, P["grad"], BF, 1e-3,
                                                                               P["keys"], None, sp),
    }

    ids = torch.randint(0, 400_000, (16, n), device=dev)
    cslots = torch.empty(n, dtype=torch.int64, device=dev)
    cache_entries = {"ce_cache_prepare_ids (zero-copy)": _lib.CE_TRANSPORT_ZEROCOPY,
                     "ce_cache_prepare_ids_begin_padded + _finish (worker)": _lib.CE_TRANSPORT_WORKER}
    entries.update(dict.fromkeys(cache_entries))

    def burst_us(call, L, reps=40, bursts=20):
        per = []
        for _ in range(bursts):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                call(L)
            per.append((time.perf_counter() - t0) / reps * 1e6)
        torch.cuda.synchronize()
        return statistics.median(per)

    for name, call in entries.items():
        for L in libs.values():                       # once, untimed: module load, and every call must succeed
            assert call is None or call(L) == _lib.CE_OK, (name, L.ce_last_error())
        torch.cuda.synchronize()
        rounds = {k: [] for k in libs}
        for _ in range(5):
            for k, L in libs.items():
                if call is None:                      # a cache op: a full cache of its own (its fill asserts every call)
                    cache = Cache(L, cache_entries[name], ids, cslots.data_ptr(), sp)
                    rounds[k].append(burst_us(lambda _L: cache.call(), L))
                    cache.close()
                else:
                    rounds[k].append(burst_us(call, L))
        aa = max(abs(a - b) for a, b in zip(rounds["parent"], rounds["parent_copy"]))
        med = {k: statistics.median(v) for k, v in rounds.items()}
        print(json.dumps({"entry": name, "us_per_call_by_round": {k: [round(x, 2) for x in v] for k, v in rounds.items()},
                          "median_us": {k: round(v, 2) for k, v in med.items()}, "largest_aa_diff_us": round(aa, 2),
                          "branch_minus_parent_us": round(med["branch"] - med["parent"], 2),
                          "pass": abs(med["branch"] - med["parent"]) <= aa}), flush=True)


if __name__ == "__main__":
    main()
