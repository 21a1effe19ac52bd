"""Backward time of the atomic fused updates with the learning rate passed by value (a float: the ce_*_act entries)
against the learning rate read from device memory (a one-element tensor: the ce_*_lrdev entries), on the same windows
(one process, device events around backward alone).

The shape of benchmarks/bench_step_accumulator.py: the package's synthetic Criteo-shaped tables (configs[2] = criteo_1tb
at --table_scale 1.0; default 0.1), B = 16384, F = 26, D = 128, a 1 % cache, prefetch window P = 8, the backward from
the window's source-row keys.  Two update kinds on an fp32 table, one module each: SGD (k_bag_bwd_stream alone) and
row-wise Adagrad (mark, k_bag_bwd_stream into the accumulator, k_rows_apply).  The two forms take turns batch by batch on
that module's cache, first one then the other in alternating order, with the same rate, so both fold the same lookups
into the same rows; --runs (3) blocks of --windows windows give one median each.
Prints ONE JSON line: median ms per backward of each form per run and over all runs, the ratio, and the spread (max -
min) of the by-value form's per-run medians -- the yardstick for the difference (profiles/device_lr.md)."""
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
from cachedembedding_amd import synthetic  # noqa: E402
from cachedembedding_amd.pipeline import PrefetchWindow  # noqa: E402

FORMS = ("value", "device")
KINDS = (("fp32_sgd", "sgd"), ("fp32_adagrad", "adagrad"))


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
    p.add_argument("--kinds", default="fp32_sgd,fp32_adagrad")
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
    lr_t = torch.full((1,), a.lr, dtype=torch.float32, device=dev)
    res = {"bench": "bench_device_lr", "dataset": a.dataset, "table_scale": a.table_scale, "num_embeddings": N,
           "cuda_row_num": C, "batch_size": B, "features": F, "dim": D, "prefetch_num": P, "runs": a.runs,
           "windows_per_run": a.windows,
           "scope": "backward alone, from the window's source-row keys (device events around out.backward); forward "
                    "and cache op outside the timed range"}
    for name, opt in KINDS:
        if name not in a.kinds.split(","):
            continue
        gen = synthetic.SyntheticKJT(sizes, B, 1, "power_law", 0.25, seed=a.seed, device=dev)
        emb = ce.CachedEmbeddingBag(N, D, mode="sum", include_last_offset=True, cuda_row_num=C, strict=False,
                                    init_seed=a.seed)
        emb.set_cache_op(False)
        setter = emb.set_fused_sgd if opt == "sgd" else emb.set_fused_rowwise_adagrad
        win = PrefetchWindow(emb, P, overlap=False, presort=True, bag_layout=layout)
        events = {v: [[] for _ in range(a.runs)] for v in FORMS}
        for w in range(a.warmup_windows + a.runs * a.windows):
            run = (w - a.warmup_windows) // a.windows
            values = gen.next_values(P)
            slots = win.prepare([values[i] for i in range(P)])
            for i in range(P):
                for v in (FORMS if (w + i) % 2 == 0 else FORMS[::-1]):
                    setter(lr_t if v == "device" else a.lr)
                    out = emb(slots[i], off, hook_features=F, presorted=win.keys[i])
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out.backward(grad)
                    e1.record()
                    if w >= a.warmup_windows:
                        events[v][run].append((e0, e1))
        torch.cuda.synchronize()
        r = {}
        for v in FORMS:
            per_run = [[e0.elapsed_time(e1) for e0, e1 in ev] for ev in events[v]]
            r[v + "_ms_per_run"] = [round(float(np.median(ms)), 4) for ms in per_run]
            flat = [t for ms in per_run for t in ms]
            r[v + "_ms"] = round(float(np.median(flat)), 4)
            r[v + "_ms_min_max"] = [round(float(min(flat)), 4), round(float(max(flat)), 4)]
        r["device_over_value"] = round(r["device_ms"] / r["value_ms"], 3)
        r["device_minus_value_ms"] = round(r["device_ms"] - r["value_ms"], 4)
        r["value_spread_ms"] = round(max(r["value_ms_per_run"]) - min(r["value_ms_per_run"]), 4)
        res[name] = r
        del win, emb
        torch.cuda.empty_cache()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
