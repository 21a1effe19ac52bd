"""Backward time of the deterministic row-wise Adagrad against the two backwards it sits between: the atomic row-wise
Adagrad and FusedSGD(deterministic=True), on the same slots (one process, device events around backward alone).

The package's synthetic Criteo-shaped tables (configs[2] = criteo_1tb at --table_scale 1.0; default 0.1), B = 16384,
F = 26, D = 128, a 1 % cache, prefetch window P = 8 -- the shape of benchmarks/bench_rowwise_adagrad.py.  One module per
table dtype (fp32, bf16 rounded to nearest); the variants take turns batch by batch on that module's cache, so all of them fold the same
lookups into the same rows:
  adagrad_atomic_keys    the streaming backward over the window's source-row keys (what a trainer runs)
  adagrad_atomic_slots   the same update from slots + offsets
  adagrad_deterministic  ce_bag_backward_update_sorted (slots + offsets)
  sgd_deterministic      ce_bag_backward_sgd_sorted (fp32 table only: it has no 16-bit form)
Prints ONE JSON line: median ms per backward of each, the ratios, and the bytes of both Adagrad workspaces at this
shape and at configs[2]'s cache (1779442 rows)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import cachedembedding_amd as ce  # noqa: E402
from cachedembedding_amd import _lib, synthetic  # noqa: E402
from cachedembedding_amd.pipeline import PrefetchWindow  # noqa: E402

VARIANTS = ("adagrad_atomic_keys", "adagrad_atomic_slots", "adagrad_deterministic", "sgd_deterministic")


def _select(emb, variant, lr):
    emb.set_fused_sgd(None)
    emb.set_fused_rowwise_adagrad(None)
    if variant == "sgd_deterministic":
        emb.set_fused_sgd(lr, deterministic=True)
    else:
        emb.set_fused_rowwise_adagrad(lr, deterministic=variant == "adagrad_deterministic")


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--dataset", default="criteo_1tb", choices=list(synthetic.TABLES))
    p.add_argument("--table_scale", type=float, default=0.1)
    p.add_argument("--batch_size", type=int, default=16384)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--cache_ratio", type=float, default=0.01)
    p.add_argument("--prefetch_num", type=int, default=8)
    p.add_argument("--windows", type=int, default=4, help="timed windows per table dtype")
    p.add_argument("--warmup_windows", type=int, default=1)
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--seed", type=int, default=1024)
    a = p.parse_args(argv)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sizes = synthetic.scale_tables(synthetic.TABLES[a.dataset], a.table_scale)
    N, D, B, F, P = int(sum(sizes)), a.dim, a.batch_size, len(sizes), a.prefetch_num
    C = int(N * a.cache_ratio)
    nnz = F * B
    off = torch.arange(nnz + 1, dtype=torch.int32, device=dev)
    layout = (off, True, F)
    grad = torch.randn(B, F, D, device=dev) * 1e-2
    lib = _lib.lib
    res = {"bench": "bench_deterministic_adagrad", "dataset": a.dataset, "table_scale": a.table_scale,
           "num_embeddings": N, "cuda_row_num": C, "batch_size": B, "features": F, "dim": D, "prefetch_num": P,
           "windows": a.windows, "sorted_chunk": _lib.CE_SORTED_CHUNK,
           "scope": "backward alone (device events around out.backward); forward and cache op outside the timed range"}
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        gen = synthetic.SyntheticKJT(sizes, B, 1, "power_law", 0.25, seed=a.seed, device=dev)
        emb = ce.CachedEmbeddingBag(N, D, mode="sum", include_last_offset=True, cuda_row_num=C, strict=False,
                                    init_seed=a.seed, table_dtype=dtype)
        emb.set_cache_op(False)
        emb.set_output_dtype(torch.float32)
        if dtype != torch.float32:
            emb.set_weight_rounding("nearest")      # what the deterministic form takes; the same for every variant
        win = PrefetchWindow(emb, P, overlap=False, presort=True, bag_layout=layout)
        variants = [v for v in VARIANTS if not (v == "sgd_deterministic" and dtype != torch.float32)]
        events = {v: [] for v in variants}
        uniq = []
        for w in range(a.warmup_windows + a.windows):
            values = gen.next_values(P)
            slots = win.prepare([values[i] for i in range(P)])
            for i in range(P):
                order = variants[(w + i) % len(variants):] + variants[:(w + i) % len(variants)]
                for v in order:
                    _select(emb, v, a.lr)
                    keys = win.keys[i] if v == "adagrad_atomic_keys" else None
                    out = emb(slots[i], off, hook_features=F, presorted=keys)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out.backward(grad)
                    e1.record()
                    if w >= a.warmup_windows:
                        events[v].append((e0, e1))
                if w >= a.warmup_windows and i == 0:
                    s = slots[i]
                    u, cnt = torch.unique(s[s >= 0], return_counts=True)
                    uniq.append((int(u.numel()), int(cnt.max()), int((cnt > _lib.CE_SORTED_CHUNK).sum())))
        torch.cuda.synchronize()
        r = {}
        for v in variants:
            ms = [e0.elapsed_time(e1) for e0, e1 in events[v]]
            r[v + "_ms"] = round(float(np.median(ms)), 4)
            r[v + "_ms_min_max"] = [round(float(min(ms)), 4), round(float(max(ms)), 4)]
        r["deterministic_over_atomic_keys"] = round(r["adagrad_deterministic_ms"] / r["adagrad_atomic_keys_ms"], 3)
        r["deterministic_over_atomic_slots"] = round(r["adagrad_deterministic_ms"] / r["adagrad_atomic_slots_ms"], 3)
        if "sgd_deterministic_ms" in r:
            r["deterministic_over_sgd_deterministic"] = round(r["adagrad_deterministic_ms"] / r["sgd_deterministic_ms"], 3)
        r["unique_slots_max_run_runs_over_chunk"] = uniq
        atomic_ws = lib.ce_bag_backward_rowwise_adagrad_workspace if dtype == torch.float32 \
            else lib.ce_bag_backward_w16_workspace
        r["workspace_bytes"] = {"atomic": int(atomic_ws(C, D)),
                                "deterministic": int(lib.ce_bag_backward_update_sorted_workspace(C, nnz, D)),
                                "atomic_at_1779442_rows": int(atomic_ws(1779442, D)),
                                "deterministic_at_1779442_rows":
                                    int(lib.ce_bag_backward_update_sorted_workspace(1779442, nnz, D))}
        f = emb.fused_adagrad
        r["workspace_allocated"] = {k: (None if t is None else int(t.numel()))
                                    for k, t in (("atomic_fp32", f._ws), ("atomic_w16", f._ws16),
                                                 ("deterministic", f._ws_sorted))}
        res[name] = r
        del win, emb
        torch.cuda.empty_cache()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
