"""Backward time of the atomic fused updates with the cache-sized accumulator (accumulator="cache") against the
step-sized one ("step"), on the same windows (one process, device events around backward alone).

The shape of benchmarks/bench_rowwise_adagrad.py: the package's synthetic Criteo-shaped tables (configs[2] = criteo_1tb
at --table_scale 1.0; default 0.1), B = 16384, F = 26, D = 128, a 1 % cache, prefetch window P = 8, the backward from
the window's source-row keys.  Two update kinds, one module each: row-wise Adagrad on an fp32 table and SGD on a bf16
table.  The two accumulators take turns batch by batch on that module's cache, first one then the other in alternating
order, so both fold the same lookups into the same rows; --runs (3) blocks of --windows windows give one median each.
Prints ONE JSON line: median ms per backward of each accumulator per run and over all runs, the ratio, the distinct
slots of a step, and the workspace bytes of both at this shape and at configs[2]'s cache (1779442 rows).
The yardstick is the "cache" path measured in the same process; the per-launch split comes from a kernel trace of this
script in a run of its own (profiles/step_accumulator.md)."""
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

ACCUMULATORS = ("cache", "step")
KINDS = (("fp32_adagrad", torch.float32, "adagrad"), ("bf16_sgd", torch.bfloat16, "sgd"))


def _select(emb, opt, lr, accumulator):
    if opt == "adagrad":
        emb.set_fused_rowwise_adagrad(lr, accumulator=accumulator)
    else:
        emb.set_fused_sgd(lr, accumulator=accumulator)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--dataset", default="criteo_1tb", choices=list(synthetic.TABLES))
    p.add_argument("--table_scale", type=float, default=0.1)
    p.add_argument("--batch_size", type=int, default=16384)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--cache_ratio", type=float, default=0.01)
    p.add_argument("--prefetch_num", type=int, default=8)
    p.add_argument("--runs", type=int, default=3, help="timed blocks per update kind, one median each")
    p.add_argument("--windows", type=int, default=3, help="timed windows per run")
    p.add_argument("--warmup_windows", type=int, default=1)
    p.add_argument("--kinds", default="fp32_adagrad,bf16_sgd")
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
    res = {"bench": "bench_step_accumulator", "dataset": a.dataset, "table_scale": a.table_scale, "num_embeddings": N,
           "cuda_row_num": C, "batch_size": B, "features": F, "dim": D, "prefetch_num": P, "runs": a.runs,
           "windows_per_run": a.windows,
           "scope": "backward alone, from the window's source-row keys (device events around out.backward); forward "
                    "and cache op outside the timed range"}
    for name, dtype, opt in KINDS:
        if name not in a.kinds.split(","):
            continue
        gen = synthetic.SyntheticKJT(sizes, B, 1, "power_law", 0.25, seed=a.seed, device=dev)
        emb = ce.CachedEmbeddingBag(N, D, mode="sum", include_last_offset=True, cuda_row_num=C, strict=False,
                                    init_seed=a.seed, table_dtype=dtype)
        emb.set_cache_op(False)
        emb.set_output_dtype(torch.float32)
        win = PrefetchWindow(emb, P, overlap=False, presort=True, bag_layout=layout)
        events = {v: [[] for _ in range(a.runs)] for v in ACCUMULATORS}
        uniq = []
        for w in range(a.warmup_windows + a.runs * a.windows):
            run = (w - a.warmup_windows) // a.windows
            values = gen.next_values(P)
            slots = win.prepare([values[i] for i in range(P)])
            for i in range(P):
                for v in (ACCUMULATORS if (w + i) % 2 == 0 else ACCUMULATORS[::-1]):
                    _select(emb, opt, a.lr, v)
                    out = emb(slots[i], off, hook_features=F, presorted=win.keys[i])
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out.backward(grad)
                    e1.record()
                    if w >= a.warmup_windows:
                        events[v][run].append((e0, e1))
                if w >= a.warmup_windows and i == 0:
                    s = slots[i]
                    uniq.append(int(torch.unique(s[s >= 0]).numel()))
        torch.cuda.synchronize()
        r = {}
        for v in ACCUMULATORS:
            per_run = [[e0.elapsed_time(e1) for e0, e1 in ev] for ev in events[v]]
            r[v + "_ms_per_run"] = [round(float(np.median(ms)), 4) for ms in per_run]
            flat = [t for ms in per_run for t in ms]
            r[v + "_ms"] = round(float(np.median(flat)), 4)
            r[v + "_ms_min_max"] = [round(float(min(flat)), 4), round(float(max(flat)), 4)]
        r["step_over_cache"] = round(r["step_ms"] / r["cache_ms"], 3)
        r["step_over_cache_per_run"] = [round(s / c, 3) for s, c in zip(r["step_ms_per_run"], r["cache_ms_per_run"])]
        r["distinct_slots_per_step"] = uniq
        cache_ws = lib.ce_bag_backward_rowwise_adagrad_workspace if dtype == torch.float32 \
            else lib.ce_bag_backward_w16_workspace
        r["workspace_bytes"] = {"cache": int(cache_ws(C, D)),
                                "step": int(lib.ce_bag_backward_update_compact_workspace(C, nnz, D)),
                                "cache_at_1779442_rows": int(cache_ws(1779442, D)),
                                "step_at_1779442_rows":
                                    int(lib.ce_bag_backward_update_compact_workspace(1779442, nnz, D))}
        f = emb._fused()
        r["workspace_allocated"] = {k: (None if t is None else int(t.numel()))
                                    for k, t in (("cache_fp32", getattr(f, "_ws", None) if opt == "adagrad" else None),
                                                 ("cache_w16", f._ws16), ("step", f._ws_step))}
        res[name] = r
        del win, emb
        torch.cuda.empty_cache()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
