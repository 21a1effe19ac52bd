"""Fused exact row-wise Adagrad against fused SGD on the same windows (one process, device events).

The package's synthetic Criteo-shaped tables (configs[2] = criteo_1tb at --table_scale 1.0; default 0.1), B = 16384,
F = 26, D = 128, a 1 % cache, prefetch window P = 8 with source-row keys (the streaming backward).  Two modules share nothing but the
generator's windows; the optimizers alternate window by window.  Prints ONE JSON line: lookups/s of each, ms per step,
the Adagrad backward's algorithmic bytes from the shapes; ends by checking a sample of touched rows (weight and
momentum1) against the fp64 reference."""
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


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--dataset", default="criteo_1tb", choices=list(synthetic.TABLES))
    # two host tables are pinned (one per optimizer): 182 GB at 1.0, so the default is a tenth
    p.add_argument("--table_scale", type=float, default=0.1)
    p.add_argument("--batch_size", type=int, default=16384)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--cache_ratio", type=float, default=0.01)
    p.add_argument("--prefetch_num", type=int, default=8)
    p.add_argument("--windows", type=int, default=6, help="timed windows per optimizer")
    p.add_argument("--warmup_windows", type=int, default=2)
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--check_rows", type=int, default=256)
    p.add_argument("--seed", type=int, default=1024)
    a = p.parse_args(argv)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sizes = synthetic.scale_tables(synthetic.TABLES[a.dataset], a.table_scale)
    N, D, B, F, P = int(sum(sizes)), a.dim, a.batch_size, len(sizes), a.prefetch_num
    C = int(N * a.cache_ratio)
    gen = synthetic.SyntheticKJT(sizes, B, 1, "power_law", 0.25, seed=a.seed, device=dev)
    off = torch.arange(F * B + 1, dtype=torch.int32, device=dev)
    layout = (off, True, F)
    grad = (torch.randn(B, F, D, device=dev) * 1e-2)

    def module(opt):
        emb = ce.CachedEmbeddingBag(N, D, mode="sum", include_last_offset=True, cuda_row_num=C, strict=False,
                                    init_seed=a.seed)
        emb.set_cache_op(False)
        if opt == "sgd":
            emb.set_fused_sgd(a.lr)
        else:
            emb.set_fused_rowwise_adagrad(a.lr)
        return emb, PrefetchWindow(emb, P, overlap=False, presort=True, bag_layout=layout)

    mods = {o: module(o) for o in ("sgd", "adagrad")}
    ms = {o: [] for o in mods}
    check_ids, check_before = None, None
    for w in range(a.warmup_windows + a.windows):
        values = gen.next_values(P)
        for o in (("sgd", "adagrad") if w % 2 == 0 else ("adagrad", "sgd")):
            emb, win = mods[o]
            if o == "adagrad" and w == a.warmup_windows + a.windows - 1:
                # the check: rows of this last window's first batch, before and after it trains
                v0 = values[0].cpu().numpy()
                rng = np.random.default_rng(a.seed)
                check_ids = np.unique(rng.choice(v0, a.check_rows))
            slots = win.prepare([values[i] for i in range(P)])
            if check_ids is not None and o == "adagrad" and check_before is None:
                mgr = emb.cache_weight_mgr
                ids_t = torch.from_numpy(check_ids).to(dev)
                rows = mgr.idx_map[ids_t].long()
                slot_of = mgr.inverted_cached_idx[rows].long()
                check_before = (mgr.cuda_cached_weight.detach()[slot_of].double().cpu().numpy(),
                                mgr.momentum1[rows].double().cpu().numpy(), slot_of, rows)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(P if not (check_ids is not None and o == "adagrad") else 1):
                out = emb(slots[i], off, hook_features=F, presorted=win.keys[i])
                out.backward(grad)
            e1.record()
            e1.synchronize()
            if w >= a.warmup_windows and not (check_ids is not None and o == "adagrad"):
                ms[o].append(e0.elapsed_time(e1) / P)
    # the check against fp64: the first batch of the last window, one step, on the sampled rows
    W0, M0, slot_of, rows = check_before
    emb = mods["adagrad"][0]
    mgr = emb.cache_weight_mgr
    v0 = values[0]
    go = grad.double().cpu().numpy().reshape(B, F, D).transpose(1, 0, 2).reshape(F * B, D)
    W1 = mgr.cuda_cached_weight.detach()[slot_of].double().cpu().numpy()
    M1 = mgr.momentum1[rows].double().cpu().numpy()
    v0n = v0.cpu().numpy()
    worst_w = worst_m = 0.0
    for k, i in enumerate(check_ids):
        g = go[v0n == i].sum(0)
        m = M0[k] + (g * g).sum() / D
        w = W0[k] - a.lr * g / (np.sqrt(m) + 1e-8)
        worst_m = max(worst_m, abs(M1[k] - m) / max(m, 1e-30))
        worst_w = max(worst_w, float(np.max(np.abs(W1[k] - w))) / a.lr)
    ok = worst_m < 1e-4 and worst_w < 1e-4
    nnz = F * B
    res = {"bench": "bench_rowwise_adagrad", "dataset": a.dataset, "table_scale": a.table_scale, "num_embeddings": N,
           "cuda_row_num": C, "batch_size": B, "features": F, "dim": D, "prefetch_num": P, "windows": a.windows,
           "scope": "per step: forward from the window's keys + fused backward (cache op outside the timed range)"}
    for o in ms:
        t = float(np.median(ms[o]))
        res[f"{o}_ms_per_step"] = round(t, 4)
        res[f"{o}_lookups_per_s"] = nnz / (t * 1e-3)
    res["adagrad_over_sgd_step"] = round(res["adagrad_ms_per_step"] / res["sgd_ms_per_step"], 3)
    # algorithmic bytes of the Adagrad backward at this shape (upper bound: every slot of the cache touched): keys and
    # upstream gradient read once, the accumulator written by the scatter, then per UNIQUE slot acc read + zeroed,
    # the row read + written, momentum read + written, cached_idx_map read; flags written + read
    U = min(C, nnz)
    res["adagrad_bwd_bytes_upper"] = int(nnz * 8 + nnz * D * 4 + U * D * 4 + U * (4 * D * 4 + 8 + 4) + 2 * C + nnz)
    res["check"] = {"rows": int(len(check_ids)), "max_rel_err_momentum": worst_m, "max_err_weight_over_lr": worst_w,
                    "ok": bool(ok)}
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
