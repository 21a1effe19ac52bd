#!/usr/bin/env python
"""What the eviction strategy is worth on a stream whose popularity stays put and on one where it moves: for DATASET,
LFU and LRU the unique-row hit rate and the milliseconds per prepare_ids call, one JSON line per configuration.

The stream is seeded and the same for every strategy: `--calls` calls of `--ids_per_call` ids from the long-tail
generator (oracle.cache_oracle.power_law_ids, exponent s) through a fixed permutation of the table.  "drifting": the
ids are rolled by N / 50 more every 20 calls, so what was popular stops being popular.  The cache is warmed up with the
frequency count of the whole stream (for LRU: the same rows, no counters), as a trainer with --use_freq does it.

Defaults: N = 50 000 rows, 5 % of them cached, warm-up 0.7 -- the shape the strategies were first compared at on the CPU,
small enough for the cache to turn over many times in 200 calls of 2048 ids.  `--num_embeddings 0` is a table of the
Criteo-Kaggle tables' size (33.8 M rows, 1.69 M cached): the long-tail generator concentrates with the table's size, and
the whole stream names 131 k distinct rows at s = 0.25 (1.0 M even at 65 536 ids per call), fewer than the cache holds --
nothing is ever evicted and every strategy hits alike, so at that size only the time per call says something.
`--model` also runs the CPU reference models (oracle/cache_oracle.py,
tests/lru_ref.py) on the same stream and reports their hit counts: they are counts, so they must be equal.  With
`--model_only` nothing touches the GPU.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from oracle.cache_oracle import DATASET, LFU, OracleCachedParamMgr, id_freq_map, power_law_ids  # noqa: E402

STRATEGIES = ["DATASET", "LFU", "LRU"]


def make_stream(N, calls, ids_per_call, s, drifting, seed):
    """[calls, ids_per_call] int64 ids and their frequency count"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(N)
    out = np.empty((calls, ids_per_call), dtype=np.int64)
    for c in range(calls):
        base = power_law_ids(rng, N, ids_per_call, s)
        shift = (c // 20) * (N // 50) if drifting else 0
        out[c] = perm[(base + shift) % N]
    return out, id_freq_map(out, N)


def model_counts(strategy, N, C, stream, freq, warmup_ratio):
    w = np.zeros((N, 1), dtype=np.float32)
    if strategy == "LRU":
        sys.path.insert(0, str(ROOT / "tests"))
        from lru_ref import LruOracleCachedParamMgr
        m = LruOracleCachedParamMgr(w, C)
    else:
        m = OracleCachedParamMgr(w, C, LFU if strategy == "LFU" else DATASET)
    m.reorder(freq, warmup_ratio)
    for ids in stream:
        m.prepare_ids(ids)
    return sum(m.num_hits_history), sum(m.num_miss_history)


def gpu_counts(strategy, table, C, stream, freq, warmup_ratio):
    """(hits, misses, ms per call: device events around the whole stream, no host wait in between)"""
    import torch
    import cachedembedding_amd as ce
    mgr = ce.CachedParamMgr(table, C, evict_strategy=ce.EvictionStrategy[strategy], strict=False)
    mgr.reorder(freq, warmup_ratio)
    ids = torch.from_numpy(stream).cuda()
    out = torch.empty_like(ids[0])
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for c in range(ids.shape[0]):
        mgr.prepare_ids(ids[c], out=out)
    stop.record()
    torch.cuda.synchronize()
    mgr.sync_stats()
    mgr.raise_on_failed_calls()
    return sum(mgr.num_hits_history), sum(mgr.num_miss_history), start.elapsed_time(stop) / ids.shape[0]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_embeddings", type=int, default=50000, help="0: the sum of the Criteo-Kaggle tables")
    ap.add_argument("--cache_ratio", type=float, default=0.05)
    ap.add_argument("--embedding_dim", type=int, default=32)
    ap.add_argument("--warmup_ratio", type=float, default=0.7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--ids_per_call", type=int, default=2048)
    ap.add_argument("--skews", type=float, nargs="+", default=[0.25, 0.6])
    ap.add_argument("--strategies", nargs="+", default=STRATEGIES, choices=STRATEGIES)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--model", action="store_true", help="also run the CPU reference models and compare the counts")
    ap.add_argument("--model_only", action="store_true", help="the CPU reference models alone (no GPU)")
    a = ap.parse_args(argv)
    N = a.num_embeddings
    if N == 0:
        from cachedembedding_amd import synthetic
        N = sum(synthetic.TABLES["criteo_kaggle"])
    C = int(N * a.cache_ratio)
    table = None
    if not a.model_only:
        import cachedembedding_amd as ce
        table = ce.HostTable.allocate(N, a.embedding_dim)          # one table for all runs: only its size matters
        table.tensor.zero_()
        small, small_freq = make_stream(4096, 8, 256, 0.25, False, a.seed)
        for strategy in a.strategies:                              # first launches load code objects: not timed
            gpu_counts(strategy, ce.HostTable.allocate(4096, a.embedding_dim), 256, small, small_freq, 1.0)
    for s in a.skews:
        for drifting in (False, True):
            stream, freq = make_stream(N, a.calls, a.ids_per_call, s, drifting, a.seed)
            for strategy in a.strategies:
                rec = {"bench": "lru", "strategy": strategy, "stream": "drifting" if drifting else "stationary", "s": s,
                       "num_embeddings": N, "cuda_row_num": C, "warmup_ratio": a.warmup_ratio, "calls": a.calls,
                       "ids_per_call": a.ids_per_call, "seed": a.seed}
                if not a.model_only:
                    hits, misses, ms = gpu_counts(strategy, table, C, stream, freq, a.warmup_ratio)
                    rec.update(hits=hits, misses=misses, hit_rate=round(hits / max(1, hits + misses), 4),
                               ms_per_prepare_ids=round(ms, 4))
                if a.model or a.model_only:
                    mh, mm = model_counts(strategy, N, C, stream, freq, a.warmup_ratio)
                    rec.update(model_hits=mh, model_misses=mm, model_hit_rate=round(mh / max(1, mh + mm), 4))
                    if not a.model_only:
                        rec["equals_model"] = (mh, mm) == (rec["hits"], rec["misses"])
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
