"""fp32 / bf16 / fp16 embedding TABLE on the same windows (one process, device events).

The package's synthetic Criteo-shaped tables (criteo_1tb at --table_scale 0.1 by default), B = 16384, F = 26, D = 128, a
1 % cache, prefetch window P = 8 with source-row keys.  Three modules -- one per table dtype -- share nothing but the
generator's windows.  Per window and module: the cache op (admissions and write-backs over PCIe: half the bytes with a
16-bit table) is timed on its own, then the P steps -- forward from the window's keys + the fused SGD backward -- for
every variant of the module:
    fp32 table:  output fp32 | output bf16               (fp32 atomics on the rows: what the parent commit runs)
    bf16 table:  output bf16, nearest | stochastic       (mark + scatter into the fp32 accumulator + apply)
    fp16 table:  output fp16, stochastic
Prints ONE JSON line: ms per step and per cache op with min / max, lookups/s, the bytes of host table, cache and update
workspace; ends by checking on the bf16 module (nearest) one step on sampled rows: the output bit for bit against the
cache rows, rows looked up once against cast(fp32(w) - lr * g)."""
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

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# (name, table, output, rounding)
VARIANTS = [("fp32_out_fp32", "fp32", "fp32", None), ("fp32_out_bf16", "fp32", "bf16", None),
            ("bf16_nearest", "bf16", "bf16", "nearest"), ("bf16_stochastic", "bf16", "bf16", "stochastic"),
            ("fp16_stochastic", "fp16", "fp16", "stochastic")]


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--dataset", default="criteo_1tb", choices=list(synthetic.TABLES))
    p.add_argument("--table_scale", type=float, default=0.1)
    p.add_argument("--batch_size", type=int, default=16384)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--cache_ratio", type=float, default=0.01)
    p.add_argument("--prefetch_num", type=int, default=8)
    p.add_argument("--windows", type=int, default=9, help="timed windows")
    p.add_argument("--warmup_windows", type=int, default=3)
    p.add_argument("--lr", type=float, default=2.0 ** -7)
    p.add_argument("--check_rows", type=int, default=4096)
    p.add_argument("--seed", type=int, default=1024)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("bench_table_dtype needs a HIP device (MI355X): there is no CPU fallback")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sizes = synthetic.scale_tables(synthetic.TABLES[a.dataset], a.table_scale)
    N, D, B, F, P = int(sum(sizes)), a.dim, a.batch_size, len(sizes), a.prefetch_num
    C = int(N * a.cache_ratio)
    nnz = F * B
    gen = synthetic.SyntheticKJT(sizes, B, 1, "power_law", 0.25, seed=a.seed, device=dev)
    off = torch.arange(nnz + 1, dtype=torch.int32, device=dev)
    layout = (off, True, F)
    g32 = torch.randn(B, F, D, device=dev) * 1e-2
    grads = {n: g32.to(dt) for n, dt in DTYPES.items()}

    mods = {}
    for t in ("fp32", "bf16", "fp16"):
        emb = ce.CachedEmbeddingBag(N, D, mode="sum", include_last_offset=True, cuda_row_num=C, strict=False,
                                    init_seed=a.seed, table_dtype=DTYPES[t])
        emb.set_cache_op(False)
        emb.set_fused_sgd(a.lr)
        mods[t] = (emb, PrefetchWindow(emb, P, overlap=False, presort=True, bag_layout=layout))
    ms = {v[0]: [] for v in VARIANTS}
    op_ms = {t: [] for t in mods}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return r, e0.elapsed_time(e1)

    def steps(emb, win, slots, out_name):
        for i in range(P):
            out = emb(slots[i], off, hook_features=F, presorted=win.keys[i])
            out.backward(grads[out_name])

    for w in range(a.warmup_windows + a.windows):
        values = gen.next_values(P)
        tables = list(mods)
        for t in tables[w % 3:] + tables[:w % 3]:
            emb, win = mods[t]
            slots, t_op = timed(lambda: win.prepare([values[i] for i in range(P)]))
            if w >= a.warmup_windows:
                op_ms[t].append(t_op)
            for name, tt, oo, rnd in VARIANTS:
                if tt != t:
                    continue
                emb.set_output_dtype(DTYPES[oo])
                if rnd is not None:
                    emb.set_weight_rounding(rnd, seed=a.seed)
                _, t_steps = timed(lambda: steps(emb, win, slots, oo))
                if w >= a.warmup_windows:
                    ms[name].append(t_steps / P)
    # the value check: bf16 table, nearest, one step on sampled lookups of one more window's first batch
    emb, win = mods["bf16"]
    mgr = emb.cache_weight_mgr
    emb.set_output_dtype(torch.bfloat16)
    emb.set_weight_rounding("nearest")
    values = gen.next_values(P)
    slots = win.prepare([values[i] for i in range(P)])
    s0 = slots[0].reshape(-1)
    valid = (s0 >= 0).nonzero().view(-1)
    pick = valid[torch.randperm(valid.numel(), device=dev)[:a.check_rows]]
    before = mgr.cuda_cached_weight.detach()[s0[pick]].clone()
    out = emb(slots[0], off, hook_features=F, presorted=win.keys[0])
    f, b = pick // B, pick % B                                          # lookup j = f * B + b -> out[b, f]
    fwd_ok = bool(torch.equal(out.detach()[b, f].view(torch.int16), before.view(torch.int16)))
    out.backward(grads["bf16"])
    cnt = torch.bincount(s0[valid], minlength=C)
    once = cnt[s0[pick]] == 1
    after = mgr.cuda_cached_weight.detach()[s0[pick]]
    gup = grads["bf16"].float()[b, f]
    lr32 = float(torch.tensor(a.lr, dtype=torch.float32))
    want = (before.float() - gup * lr32).to(torch.bfloat16)        # lr a power of two: the product is exact
    bwd_ok = bool(torch.equal(after[once].view(torch.int16), want[once].view(torch.int16))) and int(once.sum()) > 0
    ok = fwd_ok and bwd_ok

    res = {"bench": "bench_table_dtype", "dataset": a.dataset, "table_scale": a.table_scale, "num_embeddings": N,
           "cuda_row_num": C, "batch_size": B, "features": F, "dim": D, "prefetch_num": P, "windows": a.windows,
           "scope": "per step: forward from the window's keys + fused SGD backward; the cache op of a window apart"}
    for name, tt, oo, rnd in VARIANTS:
        t = float(np.median(ms[name]))
        res[f"{name}_ms_per_step"] = round(t, 4)
        res[f"{name}_ms_per_step_min_max"] = [round(float(min(ms[name])), 4), round(float(max(ms[name])), 4)]
        res[f"{name}_lookups_per_s"] = nnz / (t * 1e-3)
    for t in mods:
        es = 4 if t == "fp32" else 2
        res[f"{t}_cache_op_ms_per_window"] = round(float(np.median(op_ms[t])), 4)
        res[f"{t}_cache_op_ms_min_max"] = [round(float(min(op_ms[t])), 4), round(float(max(op_ms[t])), 4)]
        res[f"{t}_bytes"] = {"host_table": N * D * es, "cache": C * D * es,
                             "update_workspace": 0 if t == "fp32" else C * D * 4 + C + 256}
    res["bf16_over_fp32_step"] = round(res["bf16_stochastic_ms_per_step"] / res["fp32_out_bf16_ms_per_step"], 3)
    res["bf16_over_fp32_cache_op"] = round(res["bf16_cache_op_ms_per_window"] / res["fp32_cache_op_ms_per_window"], 3)
    res["check"] = {"lookups": int(pick.numel()), "rows_looked_up_once": int(once.sum()), "forward_bit_copy": fwd_ok,
                    "single_lookup_update_bit_equal": bwd_ok, "ok": bool(ok)}
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
